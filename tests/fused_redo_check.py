"""Helper of tests/test_gpu_fused_redo.py, run as its own process so that it
loads the library named by PTG_LIB (libptg_certfail.so: every rounding
certificate of the surface pass fails, so every surface path - round 0's
included, after it has stored its features - is shaded again by the exact
pass).  Renders one frame at 160x90x8 through ptg_render_with_features and
through the two separate entries and prints one JSON line: per output whether
the bits are equal, plus the redo tallies of a counting fused render."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import ptlumi_loader  # noqa: E402,F401
from ptlumi import native as N  # noqa: E402

NAMES = ("bgra", "accum", "moments", "albedo", "normal_depth")


def main():
    import numpy as np
    from ptlumi.renderer import GpuRenderer
    frame = int(sys.argv[1])
    cfg = N.RenderConfig.make(160, 90, 8, 4)
    s = N.Scene(os.path.join(ROOT, "assets"), cfg)
    s.setup_frame(frame)
    r = GpuRenderer(0)
    r.upload(s)

    def host(ts):
        return [np.ascontiguousarray(t.cpu().numpy()).view(np.uint8) for t in ts]
    bgra, acc, mom = r.render_moments(cfg, want_accum=True)
    alb, nd = r.render_features(cfg)
    r.synchronize()
    want = host((bgra, acc, mom, alb, nd))
    got = host(r.render_with_features(cfg))
    r.enable_counters(True)
    counted = host(r.render_with_features(cfg))
    r.synchronize()
    out = {"lib": os.path.basename(N.LIB_PATH), "frame": frame,
           "equal": {n: bool(np.array_equal(g, w)) for n, g, w in zip(NAMES, got, want)},
           "counted_equal": {n: bool(np.array_equal(g, w)) for n, g, w in zip(NAMES, counted, want)},
           "covered": bool((want[3].view(np.float32)[..., 3] > 0).any()),
           "redo": r.redo_stats(), "shades": int(r.counters()[5])}
    r.enable_counters(False)
    r.close()
    s.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
