"""The hoisted camera kernel of the wavefront pipeline (trace_chunk_wavefront):
at concurrency >= 1 the camera of a slot's next chunk runs on the side stream
inside the current chunk's last bounce round, into the PathSoA half and the
counts block that round leaves free, and at concurrency 2 a render's first
cameras take turns.  None of it may change a bit.

Every render here is 64x36 with set_chunk_paths(16), i.e. at most 2^16 paths
per chunk.  The chunk plan follows size_chunks: at most 65536 // npix samples
per chunk, rounded down to whole 8-sample groups (24 for the 2304 pixels of the
frame, 16 for the 3072 pixel slots of its six 32x16 tiles), the chunk count
rounded up to a multiple of the two slots, and equal chunks of whole groups:

    64 spp  -> 4 chunks of 16        (2 per slot: one hoisted camera each)
   128 spp  -> 6 chunks, 5 x 24 + 8  (3 per slot, the last one shorter)
   192 spp  -> 8 chunks of 24        (4 per slot: the parity has alternated twice)
    tiles, 64 spp -> 4 chunks of 16

test_chunk_plan asserts these counts through the timed render's camera
launches (one camera kernel per chunk)."""
import numpy as np
import pytest

from conftest import N, arrays_copy, scene_for
from oracle import Oracle
from ptlumi import distributed as D

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 64
FRAMES = [0, 450, 1400]
CHUNK_LOG2 = 16

_cache = {}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.fixture()
def hgpu(gpu):
    """The session renderer cut into 2^16-path chunks; defaults restored after."""
    gpu.set_chunk_paths(CHUNK_LOG2)
    try:
        yield gpu
    finally:
        gpu.set_chunk_paths(27)
        gpu.set_concurrency(2)
        gpu.set_pipeline("wavefront")
        gpu.enable_timing(False)


def _render(gpu, cfg, level=2, pipeline="wavefront"):
    """(radiance bits [H][W][3], BGRA bytes) of the uploaded frame."""
    gpu.set_pipeline(pipeline)
    gpu.set_concurrency(level)
    bgra, acc = gpu.render(cfg, want_accum=True)
    gpu.synchronize()
    gpu.set_pipeline("wavefront")
    gpu.set_concurrency(2)
    return _bits(acc.cpu().numpy()[..., :3]).copy(), bgra.cpu().numpy().copy()


def _frame(gpu, assets_dir, frame, spp=SPP, bounces=4, level=2, pipeline="wavefront"):
    """_render of `frame`, computed once per (frame, spp, bounces, level, pipeline).
    One scene per spp (its subframes); the bounce limit is the render's."""
    key = (frame, spp, bounces, level, pipeline)
    if key not in _cache:
        s = scene_for(assets_dir, W, H, spp, frame=frame)
        gpu.upload(s)
        _cache[key] = _render(gpu, N.RenderConfig.make(W, H, spp, bounces), level, pipeline)
    return _cache[key]


def _same(a, b, what):
    mism = int((a[0] != b[0]).any(-1).sum())
    assert mism == 0, "%s: %d/%d pixels differ" % (what, mism, a[0].shape[0] * a[0].shape[1])
    assert np.array_equal(a[1], b[1]), what


def _cameras(gpu, render):
    """Camera launches of one timed render (= its chunks), and what it returned."""
    gpu.enable_timing(True)
    try:
        out = render()
        return gpu.kernel_times()["camera"][1], out
    finally:
        gpu.enable_timing(False)


@pytest.mark.parametrize("spp,chunks", [(64, 4), (128, 6), (192, 8)])
def test_chunk_plan(hgpu, assets_dir, spp, chunks):
    """The chunk counts the other tests rely on, and a timed render (events
    around the hoisted camera on the side stream) gives the same bits."""
    s = scene_for(assets_dir, W, H, spp, frame=450)
    hgpu.upload(s)
    n, timed = _cameras(hgpu, lambda: _render(hgpu, s.cfg))
    assert n == chunks
    _same(timed, _frame(hgpu, assets_dir, 450, spp, level=0), "timed")


@pytest.mark.parametrize("frame", FRAMES)
def test_many_chunks_per_slot(hgpu, assets_dir, frame):
    """Two chunks per slot: concurrency 2 (hoisted cameras, first cameras in
    turn) = concurrency 1 (hoisted, one slot) = concurrency 0 (in order) = the
    oracle, in radiance bits and BGRA bytes."""
    c2 = _frame(hgpu, assets_dir, frame)
    _same(c2, _frame(hgpu, assets_dir, frame, level=0), "concurrency 2 vs 0")
    _same(c2, _frame(hgpu, assets_dir, frame, level=1), "concurrency 2 vs 1")
    s = scene_for(assets_dir, W, H, SPP, frame=frame)
    acc, bgra = Oracle(s.view(), s.cfg).render_rect(0, 0, W, H)
    _same(c2, (_bits(acc[..., :3]), np.array(bgra)), "concurrency 2 vs the oracle")


@pytest.mark.parametrize("spp", [128, 192])
def test_third_and_fourth_chunk_of_a_slot(hgpu, assets_dir, spp):
    """128 spp: three chunks per slot, the last shorter than the one whose
    last round hosts its camera.  192 spp: four per slot."""
    c2 = _frame(hgpu, assets_dir, 450, spp)
    _same(c2, _frame(hgpu, assets_dir, 450, spp, level=0), "concurrency 2 vs 0")
    _same(c2, _frame(hgpu, assets_dir, 450, spp, level=1), "concurrency 2 vs 1")


@pytest.mark.parametrize("bounces", [0, 1, 2, 3, 4])
def test_parity_over_max_bounces(hgpu, assets_dir, bounces):
    """rounds = bounces + 1 odd and even, and rounds < 2 (the free half is
    free from the start): concurrency 2 = concurrency 0 = the megakernel."""
    c2 = _frame(hgpu, assets_dir, 450, bounces=bounces)
    _same(c2, _frame(hgpu, assets_dir, 450, bounces=bounces, level=0), "concurrency 2 vs 0")
    _same(c2, _frame(hgpu, assets_dir, 450, bounces=bounces, pipeline="megakernel"), "wavefront vs megakernel")


def test_dead_lanes_of_partial_tiles(hgpu, assets_dir):
    """32x16 tiles of the 64x36 frame: the bottom tile row is 4 pixels high,
    its other 12 rows are dead lanes whose zero sample the sky kernel now
    writes.  All six tiles in one shard (3072 pixel slots, 4 chunks)."""
    import torch
    s = scene_for(assets_dir, W, H, SPP, frame=450)
    hgpu.upload(s)
    sh = D.TileShard(s.cfg, 32, 16, 0, 1)
    assert sh.count == 6
    n = sh.count * 32 * 16

    def tiles(level):
        hgpu.set_concurrency(level)
        acc = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        bgra, _ = hgpu.render_tiles(s.cfg, 32, 16, sh.first, sh.stride, sh.count, out_accum=acc)
        hgpu.synchronize()
        hgpu.set_concurrency(2)
        return _bits(acc.cpu().numpy()[:, :3]).copy(), bgra.cpu().numpy().copy()

    cams, c2 = _cameras(hgpu, lambda: tiles(2))
    assert cams == 4
    c0 = tiles(0)
    assert np.array_equal(c2[0], c0[0]) and np.array_equal(c2[1], c0[1])
    assert np.array_equal(tiles(2)[0], c0[0])   # and untimed
    x, y = sh.pixels()
    ok = x >= 0
    assert (~ok).sum() == 2 * 32 * 12
    partial = ok & (y >= 32)   # the live pixels of the bottom tile row
    assert partial.sum() == 64 * 4
    full = _frame(hgpu, assets_dir, 450, level=0)
    assert np.array_equal(c2[0][partial], full[0][y[partial], x[partial]])
    assert np.array_equal(c2[1][partial], full[1][y[partial], x[partial]])
    assert np.array_equal(c2[0][ok], full[0][y[ok], x[ok]])
    assert not c2[0][~ok].any()   # a dead lane's samples are +0


def test_back_to_back_renders(hgpu, assets_dir):
    """Frame 0, an upload, frame 450, an upload, frame 0 again on one context,
    none waited for before the next is queued: each equals its render alone.
    A hoisted camera must not outlive its ptg_render, nor run ahead of the
    upload that the next one reads."""
    want = {f: _frame(hgpu, assets_dir, f, level=0) for f in (0, 450)}
    outs = []
    for f in (0, 450, 0):
        s = scene_for(assets_dir, W, H, SPP, frame=f)
        hgpu.upload(s)
        bgra, acc = hgpu.render(s.cfg, want_accum=True)
        outs.append((f, bgra, acc))
    hgpu.synchronize()
    for k, (f, bgra, acc) in enumerate(outs):
        _same((_bits(acc.cpu().numpy()[..., :3]), bgra.cpu().numpy()), want[f], "render %d (frame %d)" % (k, f))
