// The film denoiser (include/pg_capi.h "denoiser"): an edge-avoiding a-trous wavelet
// (Dammertz et al. 2010) over the demodulated irradiance, steered by the first-hit albedo and normal sums and by the
// per-pixel variance of the mean as the spatial part of SVGF is (Schied et al. 2017).  The header is the definition;
// tests/denoise_ref.py restates it in float64.  float32 throughout, built with -ffp-contract=off.
//
// Per pixel three 16-byte rows: ev = (e.rgb, V), which the levels ping-pong between two buffers, and the two
// feature rows fn = (N.xyz, 1 valid / 0 invalid) and fa = (abar.rgb, 0), written once by the prepare kernel.
// One thread per pixel and level; a pixel's result depends on its own taps only, gathered in a fixed order:
// no atomics, no order dependence, two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_kernels.h"

namespace {

constexpr int DN_TX = 32, DN_TY = 8;  // block: 32 x 8 pixels, one 128-pixel row pair per wave
constexpr float DN_CUT = 80.0f;
constexpr float DN_MOD_EPS = 0.01f;

struct DenoiseLevel {
    int W, H, step;
    float sigma_l, sigma_n, sigma_a2;  // sigma_a2 = sigma_a * sigma_a
    int last;                          // the last level writes the output row (e * mod, V)
};

__device__ __forceinline__ float dnLum(const float4 &c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }

__global__ __launch_bounds__(256) void k_denoise_prepare(uint32_t npix, const float4 *__restrict__ rgbw,
                                                         const float4 *__restrict__ sumsq,
                                                         const float4 *__restrict__ albedo,
                                                         const float4 *__restrict__ normal, float4 *__restrict__ ev,
                                                         float4 *__restrict__ fn, float4 *__restrict__ fa) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    const float4 L = rgbw[i];
    const float n = L.w;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(n > 0.0f)) {  // invalid: output 0, never a tap
        ev[i] = zero;
        fn[i] = zero;
        fa[i] = zero;
        return;
    }
    const float4 S = sumsq[i], A = albedo[i], Nn = normal[i];
    const float c[3] = {L.x / n, L.y / n, L.z / n};
    const float a[3] = {A.x / n, A.y / n, A.z / n};
    float N[3] = {Nn.x / n, Nn.y / n, Nn.z / n};
    const float len = sqrtf(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
    if (len > 0.0f) {
        N[0] /= len;
        N[1] /= len;
        N[2] /= len;
    } else {
        N[0] = N[1] = N[2] = 0.0f;
    }
    const float s2[3] = {S.x, S.y, S.z};
    float e[3], v[3];
    for (int k = 0; k < 3; ++k) {
        const float mod = a[k] + DN_MOD_EPS;
        e[k] = c[k] / mod;
        // variance of the mean; a single sample has no estimate: assume 100 % error
        const float var = n >= 2.0f ? fmaxf(s2[k] / n - c[k] * c[k], 0.0f) / n : c[k] * c[k];
        v[k] = var / (mod * mod);
    }
    ev[i] = make_float4(e[0], e[1], e[2], 0.2126f * v[0] + 0.7152f * v[1] + 0.0722f * v[2]);
    fn[i] = make_float4(N[0], N[1], N[2], 1.0f);
    fa[i] = make_float4(a[0], a[1], a[2], 0.0f);
}

// the three rows of a pixel straight from memory
struct GlobalRows {
    const float4 *__restrict__ ev, *__restrict__ fn, *__restrict__ fa;
    int W;
    __device__ __forceinline__ size_t at(int x, int y) const { return (size_t)y * (size_t)W + (size_t)x; }
    __device__ __forceinline__ float4 e(int x, int y) const { return ev[at(x, y)]; }
    __device__ __forceinline__ float4 n(int x, int y) const { return fn[at(x, y)]; }
    __device__ __forceinline__ float4 a(int x, int y) const { return fa[at(x, y)]; }
};

// d_n + d_a between a pixel (Np, ap) and a tap (Nq, aq)
__device__ __forceinline__ float dnFeature(const float4 &Np, const float4 &ap, const float4 &Nq, const float4 &aq,
                                           const DenoiseLevel &lv) {
    const float dot = Np.x * Nq.x + Np.y * Nq.y + Np.z * Nq.z;
    const float dn = fmaxf(0.0f, 1.0f - dot) / lv.sigma_n;
    const float dx = ap.x - aq.x, dy = ap.y - aq.y, dz = ap.z - aq.z;
    return dn + (dx * dx + dy * dy + dz * dz) / lv.sigma_a2;
}

// One level for pixel (x, y), which lies inside the image: the variance prefilter, then the 5 x 5 pass.
// The mean is accumulated as e_p + sum w (e_q - e_p) / sum w, the same number as sum w e_q / sum w, so that a
// constant region comes back exactly.
template <class Rows>
__device__ __forceinline__ void dnLevel(const Rows &src, const DenoiseLevel &lv, int x, int y, float4 *__restrict__ out) {
    const size_t i = (size_t)y * (size_t)lv.W + (size_t)x;
    const float4 Np = src.n(x, y);
    if (Np.w == 0.0f) {
        out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 ep = src.e(x, y), ap = src.a(x, y);
    // (a) 3 x 3 at step 1, weights (1/4, 1/2, 1/4)^2, over the taps inside, valid and within the feature cut
    float vs = 0.25f * ep.w, vw = 0.25f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= lv.W || qy >= lv.H) continue;
            const float4 Nq = src.n(qx, qy);
            if (Nq.w == 0.0f) continue;
            if (!(dnFeature(Np, ap, Nq, src.a(qx, qy), lv) <= DN_CUT)) continue;
            const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            vs += k * src.e(qx, qy).w;
            vw += k;
        }
    const float tol = lv.sigma_l * sqrtf(vs / vw) + 1e-6f;
    // (b) 5 x 5 at step s with the B3 spline; the centre counts unconditionally
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float lp = dnLum(ep);
    const float wc = 0.375f * 0.375f;
    float sw = wc, sv = wc * wc * ep.w;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + lv.step * dx, qy = y + lv.step * dy;
            if (qx < 0 || qy < 0 || qx >= lv.W || qy >= lv.H) continue;
            const float4 Nq = src.n(qx, qy);
            if (Nq.w == 0.0f) continue;
            const float4 eq = src.e(qx, qy);
            const float d = dnFeature(Np, ap, Nq, src.a(qx, qy), lv) + fabsf(lp - dnLum(eq)) / tol;
            if (!(d <= DN_CUT)) continue;  // the hard cut: a feature edge is impermeable
            const float w = h[dx + 2] * h[dy + 2] * expf(-d);
            sw += w;
            sr += w * (eq.x - ep.x);
            sg += w * (eq.y - ep.y);
            sb += w * (eq.z - ep.z);
            sv += w * w * eq.w;
        }
    float4 o = make_float4(ep.x + sr / sw, ep.y + sg / sw, ep.z + sb / sw, sv / (sw * sw));
    if (lv.last) {
        o.x *= ap.x + DN_MOD_EPS;
        o.y *= ap.y + DN_MOD_EPS;
        o.z *= ap.z + DN_MOD_EPS;
    }
    out[i] = o;
}

__global__ __launch_bounds__(DN_TX *DN_TY) void k_denoise_level(DenoiseLevel lv, const float4 *__restrict__ ev,
                                                                const float4 *__restrict__ fn,
                                                                const float4 *__restrict__ fa,
                                                                float4 *__restrict__ out) {
    const int x = blockIdx.x * DN_TX + threadIdx.x, y = blockIdx.y * DN_TY + threadIdx.y;
    if (x >= lv.W || y >= lv.H) return;
    dnLevel(GlobalRows{ev, fn, fa, lv.W}, lv, x, y, out);
}

// the rows of the block's pixels and their halo of 2 * S in LDS (steps 1 and 2: 432 and 640 pixels, 20 and 30 KiB)
template <int S> struct TileRows {
    static constexpr int R = 2 * S, PW = DN_TX + 2 * R, PH = DN_TY + 2 * R;
    const float4 *ev, *fn, *fa;  // LDS, PW * PH each
    int x0, y0;                  // image position of the tile's first cell
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * PW + (x - x0); }
    __device__ __forceinline__ float4 e(int x, int y) const { return ev[at(x, y)]; }
    __device__ __forceinline__ float4 n(int x, int y) const { return fn[at(x, y)]; }
    __device__ __forceinline__ float4 a(int x, int y) const { return fa[at(x, y)]; }
};

template <int S>
__global__ __launch_bounds__(DN_TX *DN_TY) void k_denoise_level_tiled(DenoiseLevel lv, const float4 *__restrict__ ev,
                                                                      const float4 *__restrict__ fn,
                                                                      const float4 *__restrict__ fa,
                                                                      float4 *__restrict__ out) {
    using T = TileRows<S>;
    __shared__ float4 tile[3][T::PW * T::PH];
    const int x0 = (int)blockIdx.x * DN_TX - T::R, y0 = (int)blockIdx.y * DN_TY - T::R;
    // cells outside the image stay unwritten: dnLevel tests a tap's position before it reads the tap
    for (int k = threadIdx.y * DN_TX + threadIdx.x; k < T::PW * T::PH; k += DN_TX * DN_TY) {
        const int gx = x0 + k % T::PW, gy = y0 + k / T::PW;
        if (gx < 0 || gy < 0 || gx >= lv.W || gy >= lv.H) continue;
        const size_t g = (size_t)gy * (size_t)lv.W + (size_t)gx;
        tile[0][k] = ev[g];
        tile[1][k] = fn[g];
        tile[2][k] = fa[g];
    }
    __syncthreads();
    const int x = blockIdx.x * DN_TX + threadIdx.x, y = blockIdx.y * DN_TY + threadIdx.y;
    if (x >= lv.W || y >= lv.H) return;
    dnLevel(T{tile[0], tile[1], tile[2], x0, y0}, lv, x, y, out);
}

}  // namespace

void pg_launch_denoise_prepare(hipStream_t s, uint32_t width, uint32_t height, const float4 *rgbw, const float4 *sumsq,
                               const float4 *albedo, const float4 *normal, float4 *ev, float4 *fn, float4 *fa) {
    const uint32_t npix = width * height;
    hipLaunchKernelGGL(k_denoise_prepare, dim3((npix + 255u) / 256u), dim3(256), 0, s, npix, rgbw, sumsq, albedo, normal,
                       ev, fn, fa);
}

void pg_launch_denoise_level(hipStream_t s, uint32_t width, uint32_t height, int step, float sigma_l, float sigma_n,
                             float sigma_a, bool last, const float4 *ev, const float4 *fn, const float4 *fa,
                             float4 *out, bool tiled) {
    DenoiseLevel lv;
    lv.W = (int)width;
    lv.H = (int)height;
    lv.step = step;
    lv.sigma_l = sigma_l;
    lv.sigma_n = sigma_n;
    lv.sigma_a2 = sigma_a * sigma_a;
    lv.last = last ? 1 : 0;
    const dim3 grid((width + DN_TX - 1) / DN_TX, (height + DN_TY - 1) / DN_TY);
    const dim3 block(DN_TX, DN_TY);
    if (tiled && step == 1) hipLaunchKernelGGL(k_denoise_level_tiled<1>, grid, block, 0, s, lv, ev, fn, fa, out);
    else if (tiled && step == 2) hipLaunchKernelGGL(k_denoise_level_tiled<2>, grid, block, 0, s, lv, ev, fn, fa, out);
    else hipLaunchKernelGGL(k_denoise_level, grid, block, 0, s, lv, ev, fn, fa, out);
}
