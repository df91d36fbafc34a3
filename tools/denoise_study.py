"""Study (not a test): what the feature pass and the a-trous denoiser buy.

At 1280x720, frames 0 and 450: validator PSNR (2x downscale, 8-bit) of the
raw and the denoised render at 8 .. 256 spp against this renderer's own
1024-spp frame, with the time of the render, the feature pass and the
denoise (HIP events on the context's stream around each call, second run
of each; and the synchronised host wall time).

--sweep first searches a small grid of ptg_denoise_params at 16 spp (the mean
PSNR of both frames picks the row) and uses the best row for the table; the
library's defaults (ptg_denoise_params_default) are the best row of the
recorded sweep.  Without --sweep the table uses the library's defaults.

Usage: python tools/denoise_study.py [--sweep] [--out profiles/<name>]
Writes <out>/denoise_study.json.
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ptlumi_loader  # noqa: E402

P = ptlumi_loader.load()
N, V = P.native, P.validator
from ptlumi.denoise import DenoiseParams  # noqa: E402

ASSETS = os.path.join(ROOT, "assets")
W, H = 1280, 720
FRAMES = (0, 450)
SPPS = (8, 16, 32, 64, 128, 256)
REF_SPP = 1024
SWEEP_SPP = 16
GRID = {
    "iterations": (3, 4, 5),
    "sigma_color": (0.5, 1.0, 2.0, 4.0, 8.0),
    "sigma_albedo": (0.02, 0.05, 0.1, 0.2),
    "sigma_normal": (0.15, 0.3, 0.6, 1.2),
    "sigma_depth": (0.05, 0.2, 1.0),
}


def timed(fn):
    """(result, device ms, host wall ms) of the second of two runs."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - t) * 1e3


def psnr_half(ref_half, bgra):
    return float(V.validate_frame(ref_half, bgra.cpu().numpy())[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_study"))
    args = ap.parse_args()
    r = P.GpuRenderer(0)
    result = {"config": {"width": W, "height": H, "frames": FRAMES, "reference_spp": REF_SPP},
              "device": torch.cuda.get_device_name(0)}

    def scene_at(spp):
        cfg = N.RenderConfig.make(W, H, spp)
        return cfg, N.Scene(ASSETS, cfg)

    # this renderer's own 1024-spp frames, as the validator sees them
    cfg, scene = scene_at(REF_SPP)
    ref_half = {}
    static = True
    for f in FRAMES:
        scene.setup_frame(f)
        r.upload(scene, include_static=static)
        static = False
        bgra, _ = r.render(cfg)
        r.synchronize()
        ref_half[f] = V.downscale_half(V.bgra_to_rgb(bgra.cpu().numpy()))
    scene.close()

    def inputs(spp, f, scene, cfg):
        scene.setup_frame(f)
        r.upload(scene, include_static=False)
        (bgra, acc), render_ms, render_wall = timed(lambda: r.render(cfg, want_accum=True))
        (alb, nd), feat_ms, feat_wall = timed(lambda: r.render_features(cfg))
        return bgra, acc, alb, nd, {"render_ms": render_ms, "render_wall_ms": render_wall, "features_ms": feat_ms,
                                    "features_wall_ms": feat_wall}

    params = DenoiseParams.default()
    if args.sweep:
        cfg, scene = scene_at(SWEEP_SPP)
        held = {f: inputs(SWEEP_SPP, f, scene, cfg) for f in FRAMES}
        scene.close()
        rows = []
        keys = list(GRID)
        for combo in itertools.product(*(GRID[k] for k in keys)):
            p = DenoiseParams.default(**dict(zip(keys, combo)))
            ps = []
            for f in FRAMES:
                _, acc, alb, nd, _ = held[f]
                _, bgra = r.denoise(acc, alb, nd, p)
                ps.append(psnr_half(ref_half[f], bgra))
            rows.append(dict(zip(keys, combo), psnr={str(f): v for f, v in zip(FRAMES, ps)}, mean=float(np.mean(ps))))
        rows.sort(key=lambda x: -x["mean"])
        best = rows[0]
        params = DenoiseParams.default(**{k: best[k] for k in keys})
        result["sweep"] = {"spp": SWEEP_SPP, "grid": GRID, "albedo_floor": params.albedo_floor,
                           "raw": {str(f): psnr_half(ref_half[f], held[f][0]) for f in FRAMES},
                           "best": best, "rows": rows}
        print("sweep: best", best, flush=True)
    result["params"] = params.as_dict()

    table = []
    for spp in SPPS:
        cfg, scene = scene_at(spp)
        for f in FRAMES:
            bgra, acc, alb, nd, times = inputs(spp, f, scene, cfg)
            (_, den), dn_ms, dn_wall = timed(lambda: r.denoise(acc, alb, nd, params))
            row = {"spp": spp, "frame": f, "psnr_raw": psnr_half(ref_half[f], bgra),
                   "psnr_denoised": psnr_half(ref_half[f], den), "denoise_ms": dn_ms, "denoise_wall_ms": dn_wall}
            row.update(times)
            table.append(row)
            print(json.dumps(row), flush=True)
        scene.close()
    result["table"] = table
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "denoise_study.json"), "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", os.path.join(args.out, "denoise_study.json"))


if __name__ == "__main__":
    main()
