// How a render pass is cut into chunks (host only, no HIP): pg_pass.cpp's schedulers, tests/csrc/chunk_shim.cpp
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace pgh __attribute__((visibility("hidden"))) {

// one chunk of a pass: np pixels from pb (indices into the local pixel order), nl sample layers from sample_base
struct VChunk {
    uint32_t pb, np, nl, sample_base;
};

// chunks of a pass of npix pixels x spp sample layers, at most `want` paths each:
// whole sample layers over all pixels when they fit, else pixel ranges of one layer
// (layers ascend with the chunk index: a pixel's film sums are taken in chunk order)
inline std::vector<VChunk> planChunks(uint32_t npix, uint32_t spp, uint32_t want, uint32_t sample_offset) {
    std::vector<VChunk> chunks;
    if (npix == 0 || want == 0) return chunks;
    const uint32_t layersPer = std::max<uint32_t>(1, want / npix), pixPer = std::min(npix, want);
    for (uint32_t layer = 0; layer < spp;) {
        const uint32_t nl = npix > want ? 1 : std::min(layersPer, spp - layer);
        for (uint32_t pb = 0; pb < npix; pb += pixPer)
            chunks.push_back(VChunk{pb, std::min(pixPer, npix - pb), nl, sample_offset + layer});
        layer += nl;
    }
    return chunks;
}

}  // namespace pgh
