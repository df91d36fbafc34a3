#!/usr/bin/env python3
"""Fixture for the GPU-vs-shipped-build tolerance test at the metric
configuration (tests/test_gpu_shipped_tolerance.py; VERDICT r05 weak 1(iii):
the committed metric rows were only re-read, never recomputed on hardware).

For frames 0 and 450 at 1280x720 x 1024 spp, 4 bounces, the reference AS
SHIPPED (v3: -O3 -ffast-math -march=x86-64-v3, oracle/Makefile) renders the
whole frame (`render`: baseline_render's semantics, main.cc:12-46).  Kept:

  shipped_half_f<F>   validator.py's reference frame - the shipped BGRA frame
                      as RGB, downscaled 2x (validator.py:43-54) - uint8
                      360x640x3
  shipped_band_f<F>   the shipped build's averaged radiance on rows 352-368
                      (the band parity_stats.py uses for T1), float32 16x1280x3
  shipped_bgra_band_f<F>  its tonemapped bytes on the same rows

and, in shipped_band_s1024.json, the statistics of the STRICT build (which
the GPU reproduces bit for bit) against them: what the GPU test must
recompute exactly from its own frame.  Renders come from / go to the
parity_stats.py cache (--cache, default /tmp/parity_cache).

Usage: python tests/golden/make_shipped_band.py [--cache DIR]
"""
import argparse
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import parity_stats as PS  # noqa: E402

W, H, SPP, FRAMES, BAND = 1280, 720, 1024, (0, 450), (352, 368)


def validator():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "ptv", os.path.join(ROOT, "path-tracing...but-on-the-lumi-cluster_amd", "validator.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    return V


def band_stats(acc_band, bgra_band, ship_band, ship_bgra_band):
    """T2 on the band's averaged radiances, T3 on its bytes (NaN pixels counted, left out of the means)."""
    t2 = PS.within(acc_band, ship_band).all(-1)
    m_a = np.nanmean(acc_band.reshape(-1, 3).astype(np.float64), 0)
    m_s = np.nanmean(ship_band.reshape(-1, 3).astype(np.float64), 0)
    return {
        "band_pixels_within_1e-4": round(float(t2.mean()), 6),
        "band_mean_rel_diff": [round(float(x), 7) for x in np.abs(m_a - m_s) / np.abs(m_s)],
        "band_bytes_exact": round(float((bgra_band[..., :3] == ship_bgra_band[..., :3]).all(-1).mean()), 6),
        "band_nan_pixels": int(np.isnan(acc_band).any(-1).sum()),
    }


def frame_stats(V, acc, bgra, ship_half, ship_band, ship_bgra_band):
    y0, y1 = BAND
    p, good = V.validate_frame(ship_half, bgra)
    st = {"T3v_validator_psnr_db": round(float(p), 3), "T3v_validator_good": bool(good)}
    st.update(band_stats(acc[y0:y1, :, :3], bgra[y0:y1], ship_band, ship_bgra_band))
    return st


def main():
    from oracle import Reference
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="/tmp/parity_cache")
    a = ap.parse_args()
    assets = os.path.join(ROOT, "assets")
    V = validator()
    y0, y1 = BAND
    arrays, res = {}, {"width": W, "height": H, "spp": SPP, "bounces": PS.BOUNCES, "band_rows": list(BAND),
                       "shipped_build": "-O3 -ffast-math -march=x86-64-v3 (the reference Makefile's flags, portable -march)",
                       "expected_from": "the strict build (== the GPU path bit for bit) against the shipped build",
                       "frames": {}}
    for f in FRAMES:
        tag = "f%d_%dx%d_s%d" % (f, W, H, SPP)
        out = {}
        for m in ("strict", "v3"):
            r = Reference(m, W, H, SPP, PS.BOUNCES)
            out[m] = PS._cached(a.cache, "render_%s_%s" % (m, tag), lambda r=r: r.render(assets, f, timeout=6 * 3600))
        (acc_s, bgra_s), (acc_v, bgra_v) = out["strict"], out["v3"]
        ship_half = V.downscale_half(V.bgra_to_rgb(bgra_v))
        ship_band = np.ascontiguousarray(acc_v[y0:y1, :, :3])
        ship_bgra_band = np.ascontiguousarray(bgra_v[y0:y1])
        arrays["shipped_half_f%d" % f] = ship_half
        arrays["shipped_band_f%d" % f] = ship_band
        arrays["shipped_bgra_band_f%d" % f] = ship_bgra_band
        res["frames"][str(f)] = frame_stats(V, acc_s, bgra_s, ship_half, ship_band, ship_bgra_band)
        print(f, json.dumps(res["frames"][str(f)]))
    # an npz is a zip of .npy members; LZMA instead of savez_compressed's deflate keeps this one below 1 MiB
    with zipfile.ZipFile(os.path.join(HERE, "shipped_band_s1024.npz"), "w", zipfile.ZIP_LZMA) as z:
        for name, a in arrays.items():
            with z.open(name + ".npy", "w") as fh:
                np.save(fh, a)
    with open(os.path.join(HERE, "shipped_band_s1024.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
