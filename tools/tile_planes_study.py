"""Study (not a test): what the five-plane tile route costs on rank 0.

    tile_planes_study.py assemble    one JSON line
    tile_planes_study.py denoise     one JSON line per frame (0 and 450)

assemble: 1280x720 in 32x16 tiles for 8 ranks; the gathered packs hold random
bytes (the kernel copies, it needs no scene).  One ptg_assemble_tile_packs
call of all five planes between two HIP events on the context's stream,
10 calls after 3 warm-ups: median (min .. max); and bursts of 50 and 500 calls
back to back, per call the host's enqueue time, the synchronised host wall
time and the time between two events around the burst.  Next to it the 8 x 5 launches of the
per-rank, per-plane scatter the call stands in for, emulated with
ptg_scatter_tiles for the BGRA plane and a float4 copy of the rank's slots
(torch's copy_) for the other four, timed the same two ways.

denoise: 1280x720x256, frames 0 and 450: distributed.render_and_denoise at
world size 1 with its gather forced over RCCL (a process group of one)
against GpuRenderer.render_denoised_guided, synchronised host wall ms, one
warm-up each, then 3 repetitions alternating; the two results compared bit
for bit.
"""
import ctypes as C
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ptlumi_loader  # noqa: E402,F401
from ptlumi import distributed as D  # noqa: E402
from ptlumi import native as N  # noqa: E402
from ptlumi.renderer import GpuRenderer  # noqa: E402


def _stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def _timed(fn, sync, calls=10, warm=3, bursts=(50, 500)):
    """fn between two events, `calls` times; then bursts of calls back to
    back, each between two events and under a host clock that ends in a
    synchronise (ms per call: the host's enqueue alone, the wall time, the
    events)."""
    import torch
    for _ in range(warm):
        fn()
    sync()
    ev = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        sync()
        ev.append(a.elapsed_time(b))
    out = {"events_ms": _stats(ev)}
    for n in bursts:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        t = time.perf_counter()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        enqueued = time.perf_counter() - t
        sync()
        wall = time.perf_counter() - t
        out["back_to_back_%d_ms_per_call" % n] = {"enqueue": round(enqueued * 1e3 / n, 4), "wall": round(wall * 1e3 / n, 4),
                                                  "events": round(a.elapsed_time(b) / n, 4)}
    return out


def assemble():
    import torch
    w, h, tw, th, world = 1280, 720, 32, 16, 8
    cfg = N.RenderConfig.make(w, h, 256)
    r = GpuRenderer(0)
    L = N.lib()
    shard = D.TileShard(cfg, tw, th, 0, world)
    lay = D.tile_pack_layout(shard)
    packs = torch.randint(0, 256, (world, lay["bytes"]), dtype=torch.uint8, device="cuda:0")
    acc, mom, alb, nd = (torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(4))
    bgra = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())

    def one_launch():
        N.check(L.ptg_assemble_tile_packs(r._ctx, C.byref(cfg), tw, th, world, lay["pack_tiles"], p(packs), p(acc), p(bgra),
                                          p(mom), p(alb), p(nd)), "ptg_assemble_tile_packs")
    s = lay["slots"]
    floats = [[packs[k, lay[name]:lay[name] + 16 * s].view(torch.float32).view(s, 4) for name in D.PACK_PLANES[:4]]
              for k in range(world)]
    tiles = [packs[k, lay["bgra"]:lay["bgra"] + 4 * s] for k in range(world)]
    flat = [t.view(-1, 4) for t in (acc, mom, alb, nd)]
    counts = [shard.count_for(k) for k in range(world)]

    def forty_launches():
        at = 0
        for k in range(world):
            n = counts[k] * tw * th
            N.check(L.ptg_scatter_tiles(r._ctx, C.byref(cfg), tw, th, k, world, counts[k], p(tiles[k]), p(bgra)), "ptg_scatter_tiles")
            for dst, src in zip(flat, floats[k]):
                dst[at:at + n].copy_(src[:n])
            at += n
    out = {"what": "assemble", "size": [w, h], "tile": [tw, th], "world": world, "pack_bytes": lay["bytes"],
           "gathered_bytes": world * lay["bytes"], "image_bytes_written": 68 * w * h,
           "one_launch": _timed(one_launch, torch.cuda.synchronize),
           "forty_launches": _timed(forty_launches, torch.cuda.synchronize)}
    # the launch is the twin's frame at this size too
    one_launch()
    r.synchronize()
    want = D.assemble_packs_numpy(shard, packs.cpu().numpy())
    got = [t.cpu().numpy() for t in (bgra, acc, mom, alb, nd)]
    out["equals_numpy_twin"] = all(np.array_equal(g.view(np.uint8), x.view(np.uint8)) for g, x in zip(got, want))
    r.close()
    print(json.dumps(out), flush=True)


def denoise():
    import torch
    import torch.distributed as dist
    w, h, spp = 1280, 720, 256
    cfg = N.RenderConfig.make(w, h, spp)
    scene = N.Scene(os.path.join(ROOT, "assets"), cfg)
    r = GpuRenderer(0)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    stream = torch.cuda.Stream()
    r.set_stream(stream)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    shard = D.TileShard(cfg, 32, 16, 0, 1)
    try:
        for frame in (0, 450):
            scene.setup_frame(frame)
            r.upload(scene)

            def single():
                with torch.cuda.stream(stream):
                    return r.render_denoised_guided(cfg)

            def sharded():
                return D.render_and_denoise(r, cfg, shard, stream=stream)
            ms = {"render_denoised_guided": [], "render_and_denoise": []}
            for rep in range(4):   # rep 0 warms up
                for name, fn in (("render_denoised_guided", single), ("render_and_denoise", sharded)):
                    stream.synchronize()
                    t = time.perf_counter()
                    res = fn()
                    stream.synchronize()
                    if rep:
                        ms[name].append((time.perf_counter() - t) * 1e3)
                    if name == "render_denoised_guided":
                        want = [x.cpu().numpy() for x in res]
                    else:
                        equal = all(np.array_equal(g.cpu().numpy().view(np.uint8), x.view(np.uint8)) for g, x in zip(res, want))
            print(json.dumps({"what": "denoise", "size": [w, h, spp], "frame": frame, "backend": dist.get_backend(),
                              "ms": {k: _stats(v) for k, v in ms.items()}, "bits_equal": equal}), flush=True)
    finally:
        dist.destroy_process_group()
    r.close()


if __name__ == "__main__":
    {"assemble": assemble, "denoise": denoise}[sys.argv[1]]()
