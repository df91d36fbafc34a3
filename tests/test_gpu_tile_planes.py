"""The five-plane tile route on the GPU: ptg_render_tiles_packed (every rank's
tile set into one tile pack), ptg_assemble_tile_packs (the frame from the
gathered packs in one launch) and the product's render_and_gather_planes /
render_and_denoise over them.  The partition never changes a pixel, so every
expectation is bit equality with render_with_features / render_denoised_guided
of the full rectangle on one GPU.  The ranks are emulated one after the other
on the one GPU of the test machine; the collective itself runs over RCCL at
world size 1 and over gloo between two processes that share GPU 0."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, N, arrays_copy, scene_for
from ptlumi import distributed as D

pytestmark = pytest.mark.gpu

CASES = [(67, 43, 32, 16, 1), (67, 43, 32, 16, 2), (67, 43, 32, 16, 3), (67, 43, 32, 16, 8),
         (67, 43, 32, 16, 16),          # 9 tiles: ranks 9..15 hold none
         (64, 36, 8, 8, 3), (23, 11, 5, 3, 2), (23, 11, 5, 3, 7)]
FRAMES = (0, 450)
NAMES = ("bgra", "accum", "moments", "albedo+coverage", "normal+depth")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32)


def _host(tensors):
    return [t.cpu().numpy() for t in tensors]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        bad = np.argwhere((_bits(g) != _bits(w)).any(-1))
        assert len(bad) == 0, "%s, %s: %d/%d pixels differ, first (row, col) %s: got %s want %s" % (
            what, name, len(bad), g.shape[0] * g.shape[1], bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


_full = {}


def _reference(gpu, assets_dir, w, h, spp, frame):
    """(scene, render_with_features(cfg) of the full rectangle as read-only host
    arrays), rendered once per size and frame; leaves `frame` uploaded."""
    s = scene_for(assets_dir, w, h, spp, frame=frame)
    gpu.upload_arrays(arrays_copy(s))
    key = (w, h, spp, frame)
    if key not in _full:
        out = gpu.render_with_features(s.cfg)
        gpu.synchronize()
        _full[key] = _host(out)
        for a in _full[key]:
            a.setflags(write=False)
    return s, _full[key]


def _render_packs(gpu, cfg, tw, th, world):
    """Every rank's tile set into one [world][pack bytes] device buffer."""
    import torch
    lay = D.tile_pack_layout(D.TileShard(cfg, tw, th, 0, world))
    packs = torch.full((world, lay["bytes"]), 0xA5, dtype=torch.uint8, device="cuda:%d" % gpu.device)
    for r in range(world):
        sh = D.TileShard(cfg, tw, th, r, world)
        out = gpu.render_tiles_packed(cfg, tw, th, sh.first, sh.stride, sh.count, lay["pack_tiles"], out=packs[r])
        assert out.data_ptr() == packs[r].data_ptr()
    return lay, packs


def _check_packs(gpu, cfg, tw, th, world, lay, packs, full, what, against_render_tiles=True):
    """The kernel's frame, the twin's frame, the zero bytes and the BGRA route's two planes."""
    import torch
    got = gpu.assemble_tile_packs(cfg, tw, th, world, lay["pack_tiles"], packs)
    gpu.synchronize()
    got, host = _host(got), packs.cpu().numpy()
    _assert_same(got, full, what + ": assembled against render_with_features")
    _assert_same(got, D.assemble_packs_numpy(D.TileShard(cfg, tw, th, 0, world), host), what + ": kernel against its numpy twin")
    s = lay["slots"]
    for r in range(world):
        sh = D.TileShard(cfg, tw, th, r, world)
        x, y = sh.pixels()
        inside = np.zeros(s, bool)
        inside[:len(x)] = x >= 0
        pack = host[r]
        for name in D.PACK_PLANES:
            size = 4 if name == "bgra" else 16
            plane = pack[lay[name]:lay[name] + size * s].reshape(s, size)
            assert not plane[~inside].any(), (what, "rank %d: %s holds a non-zero byte outside the image's pixels" % (r, name))
        assert not pack[lay["bgra"] + 4 * s:].any(), (what, "rank %d: non-zero padding" % r)
        if not against_render_tiles or sh.count == 0:
            continue
        n = sh.count * tw * th
        acc_t = torch.empty((n, 4), dtype=torch.float32, device=packs.device)
        bgra_t, _ = gpu.render_tiles(cfg, tw, th, sh.first, sh.stride, sh.count, out_accum=acc_t)
        gpu.synchronize()
        assert np.array_equal(pack[lay["bgra"]:lay["bgra"] + 4 * n].reshape(n, 4), bgra_t.cpu().numpy()), (what, r, "bgra")
        assert np.array_equal(pack[:16 * n].view(np.uint32).reshape(n, 4), _bits(acc_t.cpu().numpy())), (what, r, "accum")


# ---- 1. emulated ranks, one process -----------------------------------------------

@pytest.mark.parametrize("w,h,tw,th,world", CASES)
def test_packed_tiles_assemble_to_the_full_frame(gpu, assets_dir, w, h, tw, th, world):
    for frame in FRAMES:
        s, full = _reference(gpu, assets_dir, w, h, 16, frame)
        lay, packs = _render_packs(gpu, s.cfg, tw, th, world)
        _check_packs(gpu, s.cfg, tw, th, world, lay, packs, full, "%dx%d %dx%d world %d frame %d" % (w, h, tw, th, world, frame))
        assert (full[3][..., 3] > 0).any(), "frame %d shows no surface: the feature planes would be constants" % frame


# ---- 2. chunk borders and modes ------------------------------------------------------

def test_chunk_borders_concurrency_levels_and_the_megakernel(gpu, assets_dir):
    """67x43x64 in 32x16 tiles for 2 ranks with chunks of at most 2^16 paths:
    a rank's 5 (or 4) tiles are 163840 (131072) paths, about three chunks, so
    the radiance, moment and feature folds carry across chunks under a tile
    PixelMap.  At concurrency 0 and 2 and under the megakernel pipeline the
    frame is render_with_features' of the full rectangle (default settings)."""
    w, h, tw, th, world = 67, 43, 32, 16, 2
    for frame in FRAMES:
        s, full = _reference(gpu, assets_dir, w, h, 64, frame)
        got = {}
        try:
            gpu.set_chunk_paths(16)
            for level in (0, 2):
                gpu.set_concurrency(level)
                gpu.enable_timing(True)
                got["concurrency %d" % level] = _render_packs(gpu, s.cfg, tw, th, world)
                gpu.synchronize()
                chunks = gpu.kernel_times()["camera"][1]      # one camera launch per chunk
                gpu.enable_timing(False)
                assert chunks >= 2 * world, "each rank's tile set must take several chunks, the two took %d" % chunks
            gpu.set_pipeline("megakernel")
            got["megakernel"] = _render_packs(gpu, s.cfg, tw, th, world)
            gpu.synchronize()
        finally:
            gpu.enable_timing(False)
            gpu.set_pipeline("wavefront")
            gpu.set_concurrency(2)
            gpu.set_chunk_paths(27)
        for what, (lay, packs) in got.items():
            _check_packs(gpu, s.cfg, tw, th, world, lay, packs, full, "frame %d, %s" % (frame, what), against_render_tiles=False)


# ---- 3. refusals -------------------------------------------------------------------

def test_refusals_return_their_codes_and_write_nothing(gpu, assets_dir, native_lib):
    import torch
    w, h, tw, th, world = 67, 43, 32, 16, 2
    s, _ = _reference(gpu, assets_dir, w, h, 16, 450)
    cfg = s.cfg
    dev = torch.device("cuda", gpu.device)
    lay = D.tile_pack_layout(D.TileShard(cfg, tw, th, 0, world))
    assert lay["pack_tiles"] == 5
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    INVALID, RANGE = -1, -6

    # ptg_render_tiles_packed
    pack = torch.full((lay["bytes"] + 256,), 0x5A, dtype=torch.uint8, device=dev)

    def render(tw_=tw, th_=th, first=0, stride=world, count=5, pack_tiles=5, ptr=p(pack), cfg_=cfg):
        return native_lib.ptg_render_tiles_packed(gpu._ctx, C.byref(cfg_), tw_, th_, first, stride, count, pack_tiles, ptr)
    assert render(pack_tiles=4) == INVALID and b"pack of 4 tiles for 5" in native_lib.ptg_last_error()
    assert render(ptr=None) == INVALID and b"null pack" in native_lib.ptg_last_error()
    for off in (4, 8, 1):
        assert render(ptr=p(pack, off)) == INVALID and b"16-byte aligned" in native_lib.ptg_last_error()
    assert render(tw_=0) == INVALID and render(th_=0) == INVALID and render(stride=0) == INVALID      # tile_map
    assert render(first=1, count=5) == RANGE and b"tile index beyond" in native_lib.ptg_last_error()   # tile 9 of 9
    assert render(count=6, pack_tiles=6) == RANGE
    assert render(cfg_=N.RenderConfig.make(w, h, 4096)) == RANGE and b"subframes" in native_lib.ptg_last_error()   # check_cfg
    assert render(cfg_=N.RenderConfig.make(0, h, 16)) == INVALID
    gpu.synchronize()
    assert (pack == 0x5A).all().item()

    # ptg_assemble_tile_packs
    packs = torch.full((world * lay["bytes"] + 256,), 0x5A, dtype=torch.uint8, device=dev)
    acc, mom, alb, nd = (torch.full((h, w, 4), -7.0, dtype=torch.float32, device=dev) for _ in range(4))
    bgra = torch.full((h, w, 4), 93, dtype=torch.uint8, device=dev)
    ok = dict(accum=p(acc), bgra=p(bgra), moments=p(mom), albedo=p(alb), normal_depth=p(nd))

    def assemble(world_=world, pack_tiles=5, src=p(packs), tw_=tw, **outs):
        o = dict(ok, **outs)
        return native_lib.ptg_assemble_tile_packs(gpu._ctx, C.byref(cfg), tw_, th, world_, pack_tiles, src, o["accum"], o["bgra"],
                                                  o["moments"], o["albedo"], o["normal_depth"])
    none = dict(accum=None, bgra=None, moments=None, albedo=None, normal_depth=None)
    assert assemble(**none) == INVALID and b"no output" in native_lib.ptg_last_error()
    assert assemble(moments=p(acc)) == INVALID and b"same buffer" in native_lib.ptg_last_error()
    assert assemble(normal_depth=p(alb)) == INVALID
    # an output inside the packs, one that ends inside them and one that begins inside them
    assert assemble(accum=p(packs, 256)) == INVALID and b"overlaps the packs" in native_lib.ptg_last_error()
    big = torch.full((world * lay["bytes"] + 2 * h * w * 16,), 0x5A, dtype=torch.uint8, device=dev)
    inner = h * w * 16
    assert assemble(src=p(big, inner), albedo=p(big, 256)) == INVALID and b"overlaps" in native_lib.ptg_last_error()
    assert assemble(src=p(big, inner), **dict(none, bgra=p(big, inner + world * lay["bytes"] - 4))) == INVALID
    assert assemble(world_=0) == INVALID and b"world size 0" in native_lib.ptg_last_error()
    assert assemble(src=None) == INVALID and b"null packs" in native_lib.ptg_last_error()
    assert assemble(src=p(packs, 8)) == INVALID and b"16-byte aligned" in native_lib.ptg_last_error()
    assert assemble(pack_tiles=4) == RANGE and b"largest rank holds 5" in native_lib.ptg_last_error()
    assert assemble(world_=1, pack_tiles=8) == RANGE                 # one rank holds all 9 tiles
    assert assemble(tw_=0) == INVALID
    gpu.synchronize()
    for t in (acc, mom, alb, nd):
        assert (t == -7.0).all().item()
    assert (bgra == 93).all().item() and (packs == 0x5A).all().item() and (big == 0x5A).all().item()
    # an output right behind the packs is no overlap, and a single output is enough
    packs.zero_()
    tail = torch.full((world * lay["bytes"] + h * w * 4,), 0x5A, dtype=torch.uint8, device=dev)
    tail[:world * lay["bytes"]] = 0
    assert assemble(src=p(tail), **dict(none, bgra=p(tail, world * lay["bytes"]))) == 0
    gpu.synchronize()
    assert not tail.any().item()                                        # the bytes of zeroed packs
    assert (acc == -7.0).all().item()


# ---- 4. the collective itself ----------------------------------------------------------

def test_planes_and_denoise_over_rccl(gpu, assets_dir):
    """render_and_gather_planes and render_and_denoise with the gather forced
    over RCCL (torch.distributed 'nccl') on a world-size-1 group, as
    tests/test_gpu_distributed.py does for the BGRA route: dist.gather runs on
    the device stream exactly as on 8 GPUs (RCCL cannot put two ranks on one
    GPU)."""
    import torch
    import torch.distributed as dist
    from ptlumi.denoise import DenoiseParams
    s, full = _reference(gpu, assets_dir, 160, 90, 16, 450)
    cfg = s.cfg
    want_guided = _host(gpu.render_denoised_guided(cfg))
    want_plain = _host(gpu.render_denoised(cfg))
    gpu.synchronize()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    stream = torch.cuda.Stream()
    gpu.set_stream(stream)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        assert dist.get_backend() == "nccl"
        shard = D.TileShard(cfg, 32, 16, 0, 1)
        planes = D.render_and_gather_planes(gpu, cfg, shard, stream=stream)
        guided = D.render_and_denoise(gpu, cfg, shard, stream=stream)
        plain = D.render_and_denoise(gpu, cfg, shard, params=DenoiseParams.default(), stream=stream)
        stream.synchronize()
        _assert_same(_host(planes), full, "gathered over RCCL")
        _assert_same(_host(guided), want_guided, "render_and_denoise against render_denoised_guided")
        _assert_same(_host(plain), want_plain, "render_and_denoise(DenoiseParams) against render_denoised")
    finally:
        dist.destroy_process_group()
        gpu.set_stream(torch.cuda.default_stream())


@pytest.mark.timeout(240)
def test_two_processes_gather_planes_and_denoise_on_gpu(gpu, assets_dir, tmp_path):
    """Two processes that share GPU 0, each a real GpuRenderer with its tile
    set of 160x90x16, gathered over a gloo group (through host memory) and
    assembled and denoised by rank 0.  Each child runs under its own
    `timeout -k 10`; both exit statuses are checked before anything else is
    done, and nothing more is started after a non-zero one."""
    w, h, spp, frame, tw, th = 160, 90, 16, 450, 32, 16
    s, full = _reference(gpu, assets_dir, w, h, spp, frame)
    want = _host(gpu.render_denoised_guided(s.cfg))
    gpu.synchronize()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    out = str(tmp_path / "planes.npz")
    script = os.path.join(ROOT, "tests", "tile_planes_rank.py")
    children = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, script, str(rank), "2", str(port), out] +
                                 [str(v) for v in (w, h, spp, frame, tw, th)],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(2)]
    logs = [c.communicate()[0] for c in children]
    status = [c.returncode for c in children]
    assert status == [0, 0], "rank exit statuses %s\n%s" % (status, "\n".join(l[-3000:] for l in logs))
    with np.load(out) as z:
        got = [z["arr_%d" % k] for k in range(7)]
    _assert_same(got[:5], full, "two processes over gloo")
    _assert_same(got[5:], want, "two processes: denoised against render_denoised_guided")
