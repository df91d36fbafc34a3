"""Helper of tests/test_gpu_tile_planes.py: ONE rank of a tile shard as its own
process (the test starts each under its own `timeout`).  The rank joins a gloo
group, renders its tiles of one frame on GPU 0 with a real GpuRenderer and
runs the product's render_and_gather_planes and render_and_denoise; rank 0
saves the five gathered images and the denoised pair.

    tile_planes_rank.py RANK WORLD PORT OUT.npz WIDTH HEIGHT SPP FRAME TILE_W TILE_H
"""
import datetime
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import ptlumi_loader  # noqa: E402,F401
from ptlumi import native as N  # noqa: E402


def main():
    import numpy as np
    import torch
    import torch.distributed as dist
    from ptlumi import distributed as D
    from ptlumi.renderer import GpuRenderer
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    out = sys.argv[4]
    w, h, spp, frame, tw, th = (int(a) for a in sys.argv[5:11])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        cfg = N.RenderConfig.make(w, h, spp)
        s = N.Scene(os.path.join(ROOT, "assets"), cfg)
        s.setup_frame(frame)
        r = GpuRenderer(0)
        stream = torch.cuda.Stream(0)
        r.set_stream(stream)
        r.upload(s)
        shard = D.TileShard(cfg, tw, th, rank, world)
        planes = D.render_and_gather_planes(r, cfg, shard, stream=stream)
        denoised = D.render_and_denoise(r, cfg, shard, stream=stream)
        stream.synchronize()
        if rank == 0:
            np.savez(out, *[t.cpu().numpy() for t in planes + denoised])
        else:
            assert planes is None and denoised is None
        r.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
