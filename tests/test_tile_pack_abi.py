"""The tile pack (include/ptg.h: a tile shard's five planes in one buffer)
exists at every layer that needs no GPU: the header declares the three
entries, both libraries export them, native.py binds them, ptg_tile_pack_bytes
is the documented formula and distributed.tile_pack_layout agrees with it."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT, N
from ptlumi import distributed as D

ENTRIES = ("ptg_tile_pack_bytes", "ptg_render_tiles_packed", "ptg_assemble_tile_packs")
HEADER = os.path.join(ROOT, "include", "ptg.h")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def _formula(tw, th, pack_tiles):
    slots = tw * th * pack_tiles
    if tw == 0 or th == 0 or pack_tiles == 0 or slots >= 1 << 31:
        return 0
    return (68 * slots + 255) // 256 * 256


def test_the_header_declares_the_entries_and_the_abi_version_stays(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in ENTRIES:
        assert re.search(r"\b%s\s*\(" % f, text), f
    assert native_lib.ptg_abi_version() == 1


def test_both_libraries_export_them():
    certfail = os.path.join(os.path.dirname(N.LIB_PATH), "libptg_certfail.so")
    for path in (N.LIB_PATH, certfail):
        missing = [f for f in ENTRIES if f not in _exports(path)]
        assert not missing, (path, missing)


def test_native_binds_them(native_lib):
    U32, P, I = C.c_uint32, C.c_void_p, C.c_int
    assert native_lib.ptg_tile_pack_bytes.restype is C.c_size_t
    assert list(native_lib.ptg_tile_pack_bytes.argtypes) == [U32] * 3
    assert list(native_lib.ptg_render_tiles_packed.argtypes) == [P, P] + [U32] * 6 + [P]
    assert list(native_lib.ptg_assemble_tile_packs.argtypes) == [P, P] + [U32] * 4 + [P] * 6
    for f in ENTRIES[1:]:
        assert getattr(native_lib, f).restype is I


@pytest.mark.parametrize("tw,th,pack_tiles,want", [
    (32, 16, 5, 174080),          # 68 * 2560, a multiple of 256 already
    (5, 3, 1, 1024),              # 68 * 15 = 1020 is no multiple of 16: padded
    (8, 8, 0, 0), (0, 8, 3, 0), (8, 0, 3, 0),
    (1, 1, 1, 256),
    (1 << 16, 1 << 15, 1, 0),     # 2^31 slots
    (1 << 16, 1 << 16, 1 << 16, 0),   # 2^48: no 32- or 64-bit wrap-around to a small size
    (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0),
    (1 << 15, 1 << 15, 1, 68 << 30),  # 2^30 slots: the size needs more than 32 bits
])
def test_pack_bytes_is_the_formula(native_lib, tw, th, pack_tiles, want):
    assert _formula(tw, th, pack_tiles) == want
    got = native_lib.ptg_tile_pack_bytes(tw, th, pack_tiles)
    assert got == want and got % 256 == 0


@pytest.mark.parametrize("w,h,tw,th,world", [(67, 43, 32, 16, 1), (67, 43, 32, 16, 2), (67, 43, 32, 16, 16), (64, 36, 8, 8, 3),
                                             (23, 11, 5, 3, 2), (23, 11, 5, 3, 7), (1280, 720, 32, 16, 8)])
def test_the_python_layout_agrees_with_the_library(native_lib, w, h, tw, th, world):
    cfg = N.RenderConfig.make(w, h, 8)
    for rank in (0, world - 1):        # the layout is the shard's, not the rank's
        lay = D.tile_pack_layout(D.TileShard(cfg, tw, th, rank, world))
        total = -(-w // tw) * -(-h // th)
        assert lay["pack_tiles"] == -(-total // world)
        s = lay["slots"]
        assert s == lay["pack_tiles"] * tw * th
        assert [lay[name] for name in D.PACK_PLANES] == [0, 16 * s, 32 * s, 48 * s, 64 * s]
        assert D.PACK_PLANES == ("accum", "moments", "albedo", "normal_depth", "bgra")
        assert lay["bytes"] == native_lib.ptg_tile_pack_bytes(tw, th, lay["pack_tiles"]) == _formula(tw, th, lay["pack_tiles"])
        assert lay["bgra"] + 4 * s <= lay["bytes"] and lay["bytes"] % 256 == 0


def test_the_entries_reject_a_null_context(native_lib):
    cfg = N.RenderConfig.make(16, 9, 8)
    assert native_lib.ptg_render_tiles_packed(None, C.byref(cfg), 8, 8, 0, 1, 1, 1, None) == -1
    assert native_lib.ptg_assemble_tile_packs(None, C.byref(cfg), 8, 8, 1, 4, None, None, None, None, None, None) == -1


def test_the_renderer_and_the_distributed_module_have_the_route():
    from ptlumi.renderer import GpuRenderer
    p = inspect.signature(GpuRenderer.render_tiles_packed).parameters
    assert list(p) == ["self", "cfg", "tile_w", "tile_h", "first", "stride", "count", "pack_tiles", "out"]
    assert p["out"].default is None
    assert list(inspect.signature(GpuRenderer.assemble_tile_packs).parameters) == [
        "self", "cfg", "tile_w", "tile_h", "world", "pack_tiles", "packs"]
    p = inspect.signature(D.render_and_gather_planes).parameters
    assert list(p) == ["renderer", "cfg", "shard", "stream", "force_collective"]
    assert p["stream"].default is None and p["force_collective"].default is True
    p = inspect.signature(D.render_and_denoise).parameters
    assert list(p)[:4] == ["renderer", "cfg", "shard", "params"] and p["params"].default is None
    # the existing route keeps its signature
    assert list(inspect.signature(D.render_and_gather).parameters) == ["renderer", "cfg", "shard", "image", "stream",
                                                                       "force_collective"]
