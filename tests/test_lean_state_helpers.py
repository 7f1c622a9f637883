"""The helpers the lean path state rests on (csrc/pg_layout.h), compiled for the host: pg_ray_tmin, the one expression
of a bounce ray's tmin (shadeOne's box test and the ray_o.w it stores), and pg_prev_front, which the writing vertex
evaluates instead of the reading vertex's dot(rd, prevRefN) >= 0.  Both must give the old expressions' bits: 1e6
random inputs and the edge inputs (zeros, denormals, a zero reference normal, grazing directions)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "lean_state_shim.cpp")
N = 1_000_000


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("leanshim") / "libleanshim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, SRC])
    L = C.CDLL(out)
    L.lean_flag_bits.restype = C.c_uint32
    L.lean_prev_front.restype = C.c_uint32
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _edge_values():
    tiny = np.float32(1e-45)  # the smallest denormal
    return np.array([0.0, -0.0, tiny, -tiny, 1e-39, -1e-39, 1.1754944e-38, 1e-4, 9.9999e-5, 1.0001e-4, 1.0, -1.0, 5.5,
                     1e-8, 3.4e38, -3.4e38], np.float32)


def test_flag_bit_is_free(shim):
    bits, f = shim.lean_flag_bits(), shim.lean_prev_front()
    assert f == 0x10 and bin(bits).count("1") == 5  # five distinct bits
    assert (0xFFFF | (bits << 16)) < 0x00800000  # depth | flags << 16 stays a denormal float


def test_tmin_helper_matches_the_old_expression(shim):
    rng = np.random.default_rng(11)
    p = (rng.standard_normal((N, 3)) * np.exp(rng.uniform(-25, 12, (N, 1)))).astype(np.float32)
    e = _edge_values()
    grid = np.stack(np.meshgrid(e, e, e, indexing="ij"), -1).reshape(-1, 3)
    p = np.ascontiguousarray(np.concatenate([p, grid]), np.float32)
    new, old = np.zeros(len(p), np.float32), np.zeros(len(p), np.float32)
    shim.lean_tmin(_p(p, C.c_float), C.c_uint32(len(p)), _p(new, C.c_float), _p(old, C.c_float))
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32))
    assert (new > 0).all()  # tmin never vanishes, also at the origin
    ref = np.float32(1e-4) * np.maximum(np.abs(p).max(1), np.float32(1e-4))
    assert np.array_equal(new.view(np.uint32), ref.astype(np.float32).view(np.uint32))


def test_prev_front_matches_the_old_test(shim):
    rng = np.random.default_rng(12)
    wo = rng.standard_normal((N, 3))
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    n = rng.standard_normal((N, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    # a third of them grazing: wo almost in the plane of n, either side of it
    k = N // 3
    t = np.cross(n[:k], rng.standard_normal((k, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    wo[:k] = t + n[:k] * rng.uniform(-1e-7, 1e-7, (k, 1))
    wo[:k:5] = t[::5]  # and exactly in it, up to fp32 rounding
    n[k:k + 1000] = 0.0  # refN = 0: always front
    e = _edge_values()
    g = np.stack(np.meshgrid(e[:8], e[:8], e[:8], indexing="ij"), -1).reshape(-1, 3)
    wo = np.ascontiguousarray(np.concatenate([wo, g, g]), np.float32)
    n = np.ascontiguousarray(np.concatenate([n, g[::-1], np.zeros_like(g)]), np.float32)
    new, old = np.zeros(len(wo), np.uint8), np.zeros(len(wo), np.uint8)
    shim.lean_front(_p(wo, C.c_float), _p(n, C.c_float), C.c_uint32(len(wo)), _p(new, C.c_uint8), _p(old, C.c_uint8))
    assert np.array_equal(new, old)
    assert new[k:k + 1000].all() and new[-len(g):].all()
    assert 0.2 < new[:k].mean() < 0.8  # the grazing set falls on both sides
