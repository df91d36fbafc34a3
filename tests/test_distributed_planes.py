"""The five-plane tile route on CPU: assemble_packs_numpy (the twin of
ptg_assemble_tile_packs) places every pixel of every plane exactly once, and
the product's render_and_gather_planes runs over real gloo groups of 2 and 3
processes with a stub renderer in place of the GPU (the pattern of
tests/test_distributed.py).  Every expectation is bit equality."""
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import N
from ptlumi import distributed as D

CASES = [(67, 43, 32, 16, 1), (67, 43, 32, 16, 2), (67, 43, 32, 16, 3), (67, 43, 32, 16, 8),
         (67, 43, 32, 16, 16),          # 9 tiles: ranks 9..15 hold none
         (64, 36, 8, 8, 3), (23, 11, 5, 3, 2), (23, 11, 5, 3, 7)]
FLOAT_PLANES = D.PACK_PLANES[:4]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _value_words(plane, x, y):
    """The uint32 words a pixel's slot holds in plane number `plane`: a
    function of (x, y, plane, component) that differs between any two pixels of
    the sizes tested and between planes; as floats they include NaN patterns,
    which a copy must keep too."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    low = (y << 14) | (x << 2)                       # y < 64, x < 4096: bits 2..19
    if plane == 4:                                   # the byte plane: one word per slot
        return (low | (5 << 28) | 3).astype(np.uint32)[..., None]
    head = np.where((x + y) % 5 == 0, 0x7FC00000 | (plane << 20), (plane + 1) << 28)   # every fifth a NaN with a payload
    return (low | head).astype(np.uint32)[..., None] | np.arange(4, dtype=np.uint32)


def _stub_pack(cfg, tw, th, first, stride, count, pack_tiles):
    """What ptg_render_tiles_packed leaves for this tile set with
    _value_words as the render: a uint8 array of pack bytes, 0 outside the
    image's pixels."""
    shard = D.TileShard(cfg, tw, th, first, stride)
    lay = D.tile_pack_layout(shard)
    assert lay["pack_tiles"] == pack_tiles >= count == shard.count
    pack = np.zeros(lay["bytes"], np.uint8)
    x, y = shard.pixels()
    ok = x >= 0
    n = len(x)
    for k, name in enumerate(D.PACK_PLANES):
        words = 1 if name == "bgra" else 4
        plane = pack[lay[name]:lay[name] + 4 * words * lay["slots"]].view("<u4").reshape(-1, words)
        plane[:n][ok] = _value_words(k, x[ok], y[ok])
    return pack


def _expected(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return [_value_words(k, x, y) for k in range(5)]


def _assert_images(images, w, h, what=""):
    """images: assemble order (bgra, accum, moments, albedo, normal_depth)."""
    want = _expected(w, h)
    for name, img in zip(("bgra",) + FLOAT_PLANES, images):
        img = np.ascontiguousarray(img)
        k = D.PACK_PLANES.index(name)
        assert img.shape == (h, w, 4) and img.dtype == (np.uint8 if name == "bgra" else np.float32), (what, name)
        got = img.view(np.uint32)
        assert np.array_equal(got, want[k]), (what, name, int((got != want[k]).any(-1).sum()))


@pytest.mark.parametrize("w,h,tw,th,world", CASES)
def test_assemble_packs_numpy_places_every_pixel_once(w, h, tw, th, world):
    cfg = N.RenderConfig.make(w, h, 8)
    shard0 = D.TileShard(cfg, tw, th, 0, world)
    lay = D.tile_pack_layout(shard0)
    packs = np.stack([_stub_pack(cfg, tw, th, r, world, shard0.count_for(r), lay["pack_tiles"]) for r in range(world)])
    assert packs.shape == (world, lay["bytes"])
    if world > shard0.total:
        assert not packs[shard0.total:].any()          # ranks without a tile send zeros
    _assert_images(D.assemble_packs_numpy(shard0, packs), w, h)
    # exactly once: every image pixel has one (rank, slot) source, no two pixels share one, and the
    # sources are the slots TileShard.pixels (the scatter form) calls inside the image
    seen = np.zeros((h, w), np.int32)
    for r in range(world):
        x, y = D.TileShard(cfg, tw, th, r, world).pixels()
        ok = x >= 0
        np.add.at(seen, (y[ok], x[ok]), 1)
    assert (seen == 1).all()
    # a flat buffer and one of another rank's view give the same frame
    again = D.assemble_packs_numpy(D.TileShard(cfg, tw, th, world - 1, world), packs.reshape(-1))
    _assert_images(again, w, h)


def test_the_padding_keeps_the_second_pack_aligned():
    """One 5x3 tile per rank: 68 * 15 = 1020 bytes of planes, a stride of 1024."""
    cfg = N.RenderConfig.make(10, 3, 8)
    lay = D.tile_pack_layout(D.TileShard(cfg, 5, 3, 0, 2))
    assert (lay["slots"], lay["bgra"] + 4 * lay["slots"], lay["bytes"]) == (15, 1020, 1024)


class StubPlanesRenderer:
    """Stands in for GpuRenderer on CPU: render_tiles_packed writes
    _value_words of every pixel slot into a pack, assemble_tile_packs is the
    numpy twin of the kernel.  It also has the BGRA route's two methods, for
    the rank that calls the wrong function."""

    def __init__(self, rank):
        self.rank = rank
        self.calls = []

    def render_tiles_packed(self, cfg, tw, th, first, stride, count, pack_tiles, out=None):
        self.calls.append(("render_tiles_packed", first, stride, count, pack_tiles))
        assert out is None
        return torch.from_numpy(_stub_pack(cfg, tw, th, first, stride, count, pack_tiles))

    def assemble_tile_packs(self, cfg, tw, th, world, pack_tiles, packs):
        self.calls.append(("assemble_tile_packs", world, pack_tiles, tuple(packs.shape)))
        return tuple(torch.from_numpy(a) for a in D.assemble_packs_numpy(D.TileShard(cfg, tw, th, 0, world), packs.numpy()))

    def render_tiles(self, cfg, tw, th, first, stride, count, out_bgra=None):
        self.calls.append(("render_tiles", first, stride, count))
        return out_bgra, None

    def scatter_tiles(self, *a):
        self.calls.append(("scatter_tiles",))


def _worker(rank, world, port, w, h, tw, th, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = N.RenderConfig.make(w, h, 8)
    shard = D.TileShard(cfg, tw, th, rank, world)
    stub = StubPlanesRenderer(rank)
    got = D.render_and_gather_planes(stub, cfg, shard)          # the product function, collective included
    lay = D.tile_pack_layout(shard)
    assert stub.calls[0] == ("render_tiles_packed", rank, world, shard.count, lay["pack_tiles"])
    if rank == 0:
        assert stub.calls[1:] == [("assemble_tile_packs", world, lay["pack_tiles"], (world, lay["bytes"]))]
        np.savez(out, *[t.numpy() for t in got])
    else:
        assert got is None and len(stub.calls) == 1
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,w,h,tw,th", [(2, 67, 43, 32, 16), (3, 23, 11, 5, 3)])
def test_gather_assembles_five_planes_gloo(tmp_path, world, w, h, tw, th):
    out = str(tmp_path / "planes.npz")
    mp.spawn(_worker, args=(world, _free_port(), w, h, tw, th, out), nprocs=world, join=True)
    with np.load(out) as z:
        _assert_images([z["arr_%d" % k] for k in range(5)], w, h, "world %d" % world)


def test_without_a_group_a_one_rank_shard_is_local():
    cfg = N.RenderConfig.make(23, 11, 8)
    stub = StubPlanesRenderer(0)
    got = D.render_and_gather_planes(stub, cfg, D.TileShard(cfg, 5, 3, 0, 1))
    _assert_images([t.numpy() for t in got], 23, 11)
    assert [c[0] for c in stub.calls] == ["render_tiles_packed", "assemble_tile_packs"]
    with pytest.raises(RuntimeError, match="no process group"):
        D.render_and_gather_planes(StubPlanesRenderer(0), cfg, D.TileShard(cfg, 5, 3, 0, 2))


def _mixed_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t0 = time.monotonic()
    cfg = N.RenderConfig.make(40, 20, 8)
    shard = D.TileShard(cfg, 16, 8, rank, world)
    stub = StubPlanesRenderer(rank)
    msg = ""
    try:
        if rank == 0:     # the BGRA route on one rank, the planes route on the other
            D.render_and_gather(stub, cfg, shard, torch.zeros((20, 40, 4), dtype=torch.uint8))
        else:
            D.render_and_gather_planes(stub, cfg, shard)
    except D.ShardMismatch as e:
        msg = str(e)
    np.save(out % rank, np.array([msg, str(bool(stub.calls)), str(time.monotonic() - t0)]))
    dist.barrier()
    dist.destroy_process_group()


def test_a_rank_on_the_bgra_route_fails_every_rank(tmp_path):
    """One rank calls render_and_gather, the other render_and_gather_planes:
    the agreement carries the kind of call, so both raise ShardMismatch within
    seconds, before anything is rendered and before either gather, which
    would wait on buffers of different sizes."""
    out = str(tmp_path / "r%d.npy")
    mp.spawn(_mixed_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for r in range(2):
        msg, rendered, secs = np.load(out % r).tolist()
        assert "disagree on kind" in msg, (r, msg)
        assert rendered == "False"
        assert float(secs) < 30


def _tile_size_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = N.RenderConfig.make(40, 20, 8)
    stub = StubPlanesRenderer(rank)
    msg = ""
    try:
        D.render_and_gather_planes(stub, cfg, D.TileShard(cfg, 16 if rank == 0 else 8, 8, rank, world))
    except D.ShardMismatch as e:
        msg = str(e)
    np.save(out % rank, np.array([msg, str(bool(stub.calls))]))
    dist.barrier()
    dist.destroy_process_group()


def test_the_planes_kind_names_its_fields_as_tile_sizes(tmp_path):
    out = str(tmp_path / "r%d.npy")
    mp.spawn(_tile_size_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for r in range(2):
        msg, rendered = np.load(out % r).tolist()
        assert "disagree on tile_w" in msg and "render_and_gather_planes" in msg, (r, msg)
        assert rendered == "False"
