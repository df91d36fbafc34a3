"""Helper of tests/test_gpu_exact_fastpaths.py, run as its own process so that
it loads the library named by PTG_LIB (libptg_certfail.so: every surface path
through the exact redo pass, which keeps glibc's pow).  Renders the listed
frames at WxH x SPP, 4 bounces, through the wavefront pipeline and saves
radiance bits and BGRA of each into the npz named last.

usage: fastpaths_render.py FRAMES W H SPP OUT.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import ptlumi_loader  # noqa: E402,F401
from ptlumi import native as N  # noqa: E402


def main():
    from ptlumi.renderer import GpuRenderer
    frames = [int(f) for f in sys.argv[1].split(",")]
    w, h, spp = (int(v) for v in sys.argv[2:5])
    cfg = N.RenderConfig.make(w, h, spp, 4)
    s = N.Scene(os.path.join(ROOT, "assets"), cfg)
    r = GpuRenderer(0)
    out = {"lib": np.array(os.path.basename(N.LIB_PATH))}
    for k, f in enumerate(frames):
        s.setup_frame(f)
        r.upload(s, include_static=(k == 0))
        bgra, acc = r.render(cfg, want_accum=True)
        r.synchronize()
        out["acc_%d" % f] = np.ascontiguousarray(acc.cpu().numpy()[..., :3]).view(np.uint32)
        out["bgra_%d" % f] = bgra.cpu().numpy()
    r.close()
    s.close()
    np.savez(sys.argv[5], **out)


if __name__ == "__main__":
    main()
