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

--guided studies the variance-guided filter instead (ptg_render_moments +
ptg_denoise_guided): per row the raw, the fixed-sigma (library defaults) and
the guided PSNR, and the HIP-event times of ptg_render, ptg_render_moments and
the guided filter.  With --sweep it first ranks a grid of
ptg_denoise_guided_params by the mean guided PSNR over both frames at 16, 64
and 256 spp - one setting has to hold across sample counts - and uses the best
row; the library's defaults (ptg_denoise_guided_params_default) are the best
row of the recorded sweep.  Writes <out>/guided_study.json.

--temporal studies the temporal accumulation (ptg_temporal_accumulate through
TemporalDenoiser): for frames 0 and 450 at 8 .. 64 spp, sequences of 1, 2, 4
and 8 preceding frames with seed_stride 0 and 1; per row the raw, the
single-frame guided, the accumulated ("temporal only") and the accumulated +
guided PSNR of the target frame, the share of its pixels that found history
and the kernel's time.  Frame 0 has no preceding frames: its sequences are
frames N .. 1 played backwards, the same camera path in the other direction.
With --sweep it first ranks a grid of ptg_temporal_params times the
sigma_luminance of the guided filter that follows by the mean accumulated +
guided PSNR over both frames at 16 and 64 spp after 4 preceding frames
(seed_stride 1) and uses the best row; the library's defaults
(ptg_temporal_params_default) are the best row of the recorded sweep.  Writes
<out>/temporal_study.json.

--adaptive studies adaptive sampling (ptg_render_adaptive) against uniform
sampling of the same cost: budgets of 64, 256 and 1024 samples in 8 passes,
per row the samples taken, the active pixels per pass, time and PSNR of the
adaptive render and of ptg_render at the smallest multiple of 8 spp that takes
at least as many samples, and the cost of the machinery alone (every pixel in
every pass) against ptg_render_moments.  With --sweep it runs a grid of
threshold x dilate at budgets 64 and 256 and ranks the rows by their smallest
gain over uniform sampling of the four (frame, budget) cells; the library's
defaults (ptg_adaptive_params_default) are the best row of the recorded sweep.
Writes <out>/adaptive_study.json.

--temporal-clamp studies the two remedies DESIGN.md 4.13 names for a frame
whose camera moves (ptg_temporal_accumulate_clamped through TemporalDenoiser's
clamp_params and blur_cameras): the set-up of --temporal with seed_stride 1,
and per row four arms - today's accumulation, the frame's subframe cameras
alone (blur_cameras 8), the history clamp alone, both - each as accumulated /
accumulated + guided PSNR with the found and the clipped share of the last
frame; and the kernel's time at 1, 8 and 128 cameras (HIP events, mean of 20
calls).  With --sweep it first ranks clamp_radius x clamp_sigma x
clipped_history by the ranking rule of --temporal on the arm with both
remedies and uses the best row; the library's defaults
(ptg_temporal_clamp_params_default) are the best row of the recorded sweep.
Writes <out>/temporal_clamp_study.json.

--fused studies ptg_render_with_features (radiance, moments and features in
one pass) against the two calls it replaces: frames 0 and 450 at 8 and 256
spp, with --sweep at every sample count from 8 to 256; per row the HIP-event
times of render_moments, render_features, the two back to back and
render_with_features (the second of two runs each), what the fused pass costs
over render_moments and saves against the two calls, and whether all five
outputs had the two calls' bits.  Writes <out>/fused_study.json.

Usage: python tools/denoise_study.py [--guided | --temporal | --temporal-clamp | --adaptive | --fused] [--sweep] [--out profiles/<name>]
Writes <out>/denoise_study.json.
"""
import argparse
import itertools
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ptlumi_loader  # noqa: E402

P = ptlumi_loader.load()
N, V = P.native, P.validator
from ptlumi.denoise import DenoiseGuidedParams, DenoiseParams, TemporalClampParams, TemporalParams  # noqa: E402

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


GUIDED_SWEEP_SPPS = (16, 64, 256)
GUIDED_GRID = {
    "iterations": (3, 4, 5),
    "sigma_luminance": (0.5, 1.0, 2.0, 4.0, 8.0, 16.0),
    "sigma_albedo": (0.05, 0.2),
    "sigma_normal": (0.3, 1.2),
    "variance_floor": (1e-4, 1e-3, 1e-2),
}


def guided_study(args):
    r = P.GpuRenderer(0)
    result = {"config": {"width": W, "height": H, "frames": FRAMES, "reference_spp": REF_SPP},
              "device": torch.cuda.get_device_name(0)}
    cfg = N.RenderConfig.make(W, H, REF_SPP)
    scene = N.Scene(ASSETS, cfg)
    ref_half = {}
    for i, f in enumerate(FRAMES):
        scene.setup_frame(f)
        r.upload(scene, include_static=i == 0)
        bgra, _ = r.render(cfg)
        r.synchronize()
        ref_half[f] = V.downscale_half(V.bgra_to_rgb(bgra.cpu().numpy()))
    scene.close()

    # every (spp, frame): the render with and without the moments, timed, and the features
    held = {}
    for spp in SPPS:
        cfg = N.RenderConfig.make(W, H, spp)
        scene = N.Scene(ASSETS, cfg)
        for f in FRAMES:
            scene.setup_frame(f)
            r.upload(scene, include_static=False)
            (bgra, _), render_ms, _ = timed(lambda: r.render(cfg, want_accum=True))
            (_, acc, mom), moments_ms, _ = timed(lambda: r.render_moments(cfg, want_accum=True))
            alb, nd = r.render_features(cfg)
            r.synchronize()
            held[spp, f] = (bgra, acc, alb, nd, mom, {"render_ms": render_ms, "render_moments_ms": moments_ms})
        scene.close()

    params = DenoiseGuidedParams.default()
    if args.sweep:
        rows = []
        keys = list(GUIDED_GRID)
        cells = [(spp, f) for spp in GUIDED_SWEEP_SPPS for f in FRAMES]
        # beside the ranking, the suite's end-to-end check of every row: frame 0 at
        # 640x360x16 against the reference's own frame, full resolution (not ranked on)
        golden = np.load(os.path.join(ROOT, "tests", "golden", "frame_0000_ref.npz"))["rgb"]
        cfg = N.RenderConfig.make(640, 360, 16)
        scene = N.Scene(ASSETS, cfg)
        scene.setup_frame(0)
        r.upload(scene, include_static=False)
        e_bgra, e_acc, e_mom = r.render_moments(cfg, want_accum=True)
        e_alb, e_nd = r.render_features(cfg)
        r.synchronize()
        scene.close()
        e_raw = float(V.psnr(golden, V.bgra_to_rgb(e_bgra.cpu().numpy())))
        for combo in itertools.product(*(GUIDED_GRID[k] for k in keys)):
            p = DenoiseGuidedParams.default(**dict(zip(keys, combo)))
            ps = {}
            for spp, f in cells:
                _, acc, alb, nd, mom, _ = held[spp, f]
                _, bgra = r.denoise_guided(acc, alb, nd, mom, p)
                ps["%d@%d" % (f, spp)] = psnr_half(ref_half[f], bgra)
            _, bgra = r.denoise_guided(e_acc, e_alb, e_nd, e_mom, p)
            rows.append(dict(zip(keys, combo), psnr=ps, mean=float(np.mean(list(ps.values()))),
                             check_640x360x16_frame0=float(V.psnr(golden, V.bgra_to_rgb(bgra.cpu().numpy())))))
            if len(rows) % 30 == 0:
                print("sweep: %d rows" % len(rows), flush=True)
        rows.sort(key=lambda x: -x["mean"])
        best = rows[0]
        params = DenoiseGuidedParams.default(**{k: best[k] for k in keys})
        result["sweep"] = {"spps": GUIDED_SWEEP_SPPS, "grid": GUIDED_GRID, "fixed": {
            k: v for k, v in params.as_dict().items() if k not in keys},
            "raw": {"%d@%d" % (f, spp): psnr_half(ref_half[f], held[spp, f][0]) for spp, f in cells},
            "check_640x360x16_frame0_raw": e_raw, "best": best, "rows": rows}
        print("sweep: best", best, flush=True)
    result["params"] = params.as_dict()
    result["fixed_sigma_params"] = DenoiseParams.default().as_dict()

    table = []
    for spp in SPPS:
        for f in FRAMES:
            bgra, acc, alb, nd, mom, times = held[spp, f]
            # the filters take a fraction of a millisecond: the mean of 20 runs back to back
            (_, fixed), fixed_ms, _ = timed(lambda: [r.denoise(acc, alb, nd) for _ in range(20)][-1])
            (_, guided), guided_ms, _ = timed(lambda: [r.denoise_guided(acc, alb, nd, mom, params) for _ in range(20)][-1])
            fixed_ms, guided_ms = fixed_ms / 20, guided_ms / 20
            row = {"spp": spp, "frame": f, "psnr_raw": psnr_half(ref_half[f], bgra),
                   "psnr_fixed": psnr_half(ref_half[f], fixed), "psnr_guided": psnr_half(ref_half[f], guided),
                   "denoise_ms": fixed_ms, "denoise_guided_ms": guided_ms}
            row.update(times)
            table.append(row)
            print(json.dumps(row), flush=True)
    result["table"] = table
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "guided_study.json"), "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", os.path.join(args.out, "guided_study.json"))


TEMPORAL_SPPS = (8, 16, 32, 64)
TEMPORAL_PRECEDING = (1, 2, 4, 8)
TEMPORAL_SWEEP_SPPS = (16, 64)
TEMPORAL_SWEEP_PRECEDING = 4
TEMPORAL_GRID = {
    "max_history": (16.0, 32.0, 64.0, 128.0, 256.0),
    "depth_tolerance": (0.02, 0.05, 0.1),
    "normal_tolerance": (0.02, 0.1, 0.5),
    "albedo_tolerance": (0.01, 0.05, 0.25),
}
TEMPORAL_SIGMA_LUMINANCE = (0.5, 1.0, 2.0, 4.0)
CHECK = {"width": 320, "height": 180, "spp": 16, "reference_spp": 256, "frames": (447, 448, 449, 450)}


def sequence(frame, preceding):
    """The frames of a sequence that ends at `frame`; before frame 0 there is
    nothing, so its sequences run backwards from frame `preceding`."""
    if frame >= preceding:
        return list(range(frame - preceding, frame + 1))
    return list(range(frame + preceding, frame - 1, -1))


def dump_rows_compact(result, path):
    """json.dump(result, indent=1) with every row of the table and of the
    sweep on one line: 540 swept rows stay a few hundred lines."""
    rows = []

    def hold(row):
        rows.append(json.dumps(row))
        return "@row%d@" % (len(rows) - 1)

    doc = dict(result, table=[hold(row) for row in result["table"]])
    if "sweep" in doc:
        doc["sweep"] = dict(doc["sweep"], rows=[hold(row) for row in doc["sweep"]["rows"]])
    text = re.sub(r'"@row(\d+)@"', lambda m: rows[int(m.group(1))], json.dumps(doc, indent=1))
    with open(path, "w") as fh:
        fh.write(text + "\n")


def temporal_study(args):
    r = P.GpuRenderer(0)
    result = {"config": {"width": W, "height": H, "frames": FRAMES, "reference_spp": REF_SPP, "spps": TEMPORAL_SPPS,
                         "preceding": TEMPORAL_PRECEDING, "sequences": {str(f): sequence(f, 8) for f in FRAMES}},
              "device": torch.cuda.get_device_name(0)}
    cfg = N.RenderConfig.make(W, H, REF_SPP)
    scene = N.Scene(ASSETS, cfg)
    ref_half = {}
    for f in FRAMES:
        scene.setup_frame(f)
        r.upload(scene)
        bgra, _ = r.render(cfg)
        r.synchronize()
        ref_half[f] = V.downscale_half(V.bgra_to_rgb(bgra.cpu().numpy()))
    scene.close()

    def tonemapped(radiance):
        return r.tonemap_device(radiance, torch.empty(radiance.shape, dtype=torch.uint8, device=radiance.device))

    def frames_of(scene, cfg, frames, seed_stride):
        """Per frame of the sequence what TemporalDenoiser.step renders: (camera, radiance, moments, albedo, normal_depth)."""
        td = P.TemporalDenoiser(r, cfg, seed_stride=seed_stride)
        out = []
        for f in frames:
            scene.setup_frame(f)
            r.upload(scene)
            sub = scene.view()["subframes"]
            c = td.frame_config()
            _, acc, mom = r.render_moments(c, want_accum=True)
            out.append((N.Camera.of(sub[len(sub) // 2]["cam"]), acc, mom) + r.render_features(c))
            td.frames += 1
        return out

    def accumulate(steps, tp):
        """The sequence through ptg_temporal_accumulate, as TemporalDenoiser.step chains it (not in place)."""
        hist = None
        for cam, acc, mom, alb, nd in steps:
            rad, m, _ = r.temporal_accumulate(cam, acc, mom, alb, nd, hist, tp)
            hist = (cam, rad, m, alb, nd)
        return hist

    tparams, gparams = TemporalParams.default(), DenoiseGuidedParams.default()
    if args.sweep:
        held = {}
        for spp in TEMPORAL_SWEEP_SPPS:
            cfg = N.RenderConfig.make(W, H, spp)
            scene = N.Scene(ASSETS, cfg)
            for f in FRAMES:
                held[spp, f] = frames_of(scene, cfg, sequence(f, TEMPORAL_SWEEP_PRECEDING), 1)
            scene.close()
        # beside the ranking, the suite's end-to-end check of every row (not ranked on)
        c = CHECK
        cfg = N.RenderConfig.make(c["width"], c["height"], c["reference_spp"])
        scene = N.Scene(ASSETS, cfg)
        scene.setup_frame(c["frames"][-1])
        r.upload(scene)
        bgra, _ = r.render(cfg)
        r.synchronize()
        check_ref = V.bgra_to_rgb(bgra.cpu().numpy())
        scene.close()
        cfg = N.RenderConfig.make(c["width"], c["height"], c["spp"])
        scene = N.Scene(ASSETS, cfg)
        check_steps = frames_of(scene, cfg, c["frames"], 1)
        r.upload(scene)
        single, _ = r.render_denoised_guided(cfg)
        check_single = float(V.psnr(check_ref, V.bgra_to_rgb(single.cpu().numpy())))
        scene.close()
        rows = []
        keys = list(TEMPORAL_GRID)
        for combo in itertools.product(*(TEMPORAL_GRID[k] for k in keys)):
            tp = TemporalParams.default(**dict(zip(keys, combo)))
            acc = {cell: accumulate(steps, tp) for cell, steps in held.items()}
            chk = accumulate(check_steps, tp)
            only = {"%d@%d" % (f, spp): psnr_half(ref_half[f], tonemapped(h[1])) for (spp, f), h in acc.items()}
            for sl in TEMPORAL_SIGMA_LUMINANCE:
                gp = DenoiseGuidedParams.default(sigma_luminance=sl)
                ps = {}
                for (spp, f), h in acc.items():
                    _, bgra = r.denoise_guided(h[1], h[3], h[4], h[2], gp)
                    ps["%d@%d" % (f, spp)] = psnr_half(ref_half[f], bgra)
                _, bgra = r.denoise_guided(chk[1], chk[3], chk[4], chk[2], gp)
                rows.append(dict(zip(keys, combo), sigma_luminance=sl, psnr=ps, mean=float(np.mean(list(ps.values()))),
                                 temporal_only=only, temporal_only_mean=float(np.mean(list(only.values()))),
                                 check_frame450=float(V.psnr(check_ref, V.bgra_to_rgb(bgra.cpu().numpy())))))
            if len(rows) % 40 == 0:
                print("sweep: %d rows" % len(rows), flush=True)
        rows.sort(key=lambda x: -x["mean"])
        best = rows[0]
        tparams = TemporalParams.default(**{k: best[k] for k in keys})
        gparams = DenoiseGuidedParams.default(sigma_luminance=best["sigma_luminance"])
        result["sweep"] = {"spps": TEMPORAL_SWEEP_SPPS, "preceding": TEMPORAL_SWEEP_PRECEDING, "seed_stride": 1,
                           "grid": TEMPORAL_GRID, "sigma_luminance": TEMPORAL_SIGMA_LUMINANCE, "check": CHECK,
                           "check_single_frame_guided": check_single, "best": best, "rows": rows}
        print("sweep: best", best, "single-frame guided check", check_single, flush=True)
        del held, acc
    result["params"] = tparams.as_dict()
    result["guided_params"] = gparams.as_dict()
    result["library_guided_params"] = DenoiseGuidedParams.default().as_dict()

    table = []
    for spp in TEMPORAL_SPPS:
        cfg = N.RenderConfig.make(W, H, spp)
        scene = N.Scene(ASSETS, cfg)
        for f in FRAMES:
            scene.setup_frame(f)
            r.upload(scene)
            raw, racc, rmom = r.render_moments(cfg, want_accum=True)
            ralb, rnd = r.render_features(cfg)
            _, single = r.denoise_guided(racc, ralb, rnd, rmom)
            base = {"spp": spp, "frame": f, "psnr_raw": psnr_half(ref_half[f], raw),
                    "psnr_guided": psnr_half(ref_half[f], single)}
            for stride in (0, 1):
                for n in TEMPORAL_PRECEDING:
                    steps = frames_of(scene, cfg, sequence(f, n), stride)
                    h = accumulate(steps, tparams)
                    _, lib = r.denoise_guided(h[1], h[3], h[4], h[2])
                    _, rec = r.denoise_guided(h[1], h[3], h[4], h[2], gparams)
                    # the kernel is a fraction of a millisecond: the mean of 20 runs back to back
                    prev = accumulate(steps[:-1], tparams)
                    _, ms, _ = timed(lambda: [r.temporal_accumulate(*steps[-1], prev, tparams) for _ in range(20)][-1])
                    row = dict(base, seed_stride=stride, preceding=n, psnr_temporal=psnr_half(ref_half[f], tonemapped(h[1])),
                               psnr_temporal_guided=psnr_half(ref_half[f], rec),
                               psnr_temporal_guided_library_sigma=psnr_half(ref_half[f], lib),
                               found_history=float((h[2][..., 3] > steps[-1][2][..., 3]).float().mean()),
                               temporal_ms=ms / 20)
                    table.append(row)
                    print(json.dumps(row), flush=True)
        scene.close()
    result["table"] = table
    os.makedirs(args.out, exist_ok=True)
    dump_rows_compact(result, os.path.join(args.out, "temporal_study.json"))
    print("wrote", os.path.join(args.out, "temporal_study.json"))


CLAMP_GRID = {"clamp_radius": (1, 2), "clamp_sigma": (0.5, 1.0, 2.0, 4.0), "clipped_history": (8.0, 32.0, 128.0)}
CLAMP_BLUR_CAMERAS = 8
CLAMP_TIMED_CAMERAS = (1, 8, 128)
CLAMP_ARMS = ("today", "cameras", "clamp", "both")


def temporal_clamp_study(args):
    r = P.GpuRenderer(0)
    result = {"config": {"width": W, "height": H, "frames": FRAMES, "reference_spp": REF_SPP, "spps": TEMPORAL_SPPS,
                         "preceding": TEMPORAL_PRECEDING, "seed_stride": 1, "blur_cameras": CLAMP_BLUR_CAMERAS,
                         "arms": CLAMP_ARMS, "sequences": {str(f): sequence(f, 8) for f in FRAMES}},
              "device": torch.cuda.get_device_name(0)}
    cfg = N.RenderConfig.make(W, H, REF_SPP)
    scene = N.Scene(ASSETS, cfg)
    ref_half = {}
    for f in FRAMES:
        scene.setup_frame(f)
        r.upload(scene)
        bgra, _ = r.render(cfg)
        r.synchronize()
        ref_half[f] = V.downscale_half(V.bgra_to_rgb(bgra.cpu().numpy()))
    scene.close()

    def tonemapped(radiance):
        return r.tonemap_device(radiance, torch.empty(radiance.shape, dtype=torch.uint8, device=radiance.device))

    def frames_of(scene, cfg, frames):
        """Per frame of the sequence what TemporalDenoiser.step renders: (subframe cameras, radiance, moments, albedo,
        normal_depth)."""
        td = P.TemporalDenoiser(r, cfg, seed_stride=1)
        out = []
        for f in frames:
            scene.setup_frame(f)
            r.upload(scene)
            cams = [N.Camera.of(s["cam"]) for s in scene.view()["subframes"]]
            c = td.frame_config()
            _, acc, mom = r.render_moments(c, want_accum=True)
            out.append((cams, acc, mom) + r.render_features(c))
            td.frames += 1
        return out

    def accumulate(steps, cp, blur_cameras):
        """The sequence as TemporalDenoiser.step chains it with clamp_params `cp` and `blur_cameras` (not in place):
        (history, found share, clipped share of the last step)."""
        td = P.TemporalDenoiser(r, None, clamp_params=cp, blur_cameras=blur_cameras)
        hist, flags = None, None
        for cams, acc, mom, alb, nd in steps:
            use = [cams[k] for k in td.blur_subframes(len(cams))]
            rad, m, _, flags = r.temporal_accumulate_clamped(use, acc, mom, alb, nd, hist, cp, want_flags=True)
            hist = (cams[len(cams) // 2], rad, m, alb, nd)
        r.synchronize()
        found, clipped = r.split_flags(flags)
        return hist, float(found.float().mean()), float(clipped.float().mean())

    def arms_of(cp):
        off = TemporalClampParams.default(clamp_radius=0)
        off.base = cp.base
        return {"today": (off, 1), "cameras": (off, CLAMP_BLUR_CAMERAS), "clamp": (cp, 1), "both": (cp, CLAMP_BLUR_CAMERAS)}

    cparams, gparams = TemporalClampParams.default(), DenoiseGuidedParams.default()
    result["library_params"] = cparams.as_dict()
    if args.sweep:
        held = {}
        for spp in TEMPORAL_SWEEP_SPPS:
            cfg = N.RenderConfig.make(W, H, spp)
            scene = N.Scene(ASSETS, cfg)
            for f in FRAMES:
                held[spp, f] = frames_of(scene, cfg, sequence(f, TEMPORAL_SWEEP_PRECEDING))
            scene.close()
        rows = []
        keys = list(CLAMP_GRID)

        def cells(cp, blur_cameras):
            ps = {}
            for (spp, f), steps in held.items():
                h, _, _ = accumulate(steps, cp, blur_cameras)
                _, bgra = r.denoise_guided(h[1], h[3], h[4], h[2], gparams)
                ps["%d@%d" % (f, spp)] = psnr_half(ref_half[f], bgra)
            return ps

        off = arms_of(cparams)["today"][0]
        baseline = {"today": cells(off, 1), "cameras": cells(off, CLAMP_BLUR_CAMERAS)}
        for combo in itertools.product(*(CLAMP_GRID[k] for k in keys)):
            cp = TemporalClampParams.default(**dict(zip(keys, combo)))
            both, alone = cells(cp, CLAMP_BLUR_CAMERAS), cells(cp, 1)
            rows.append(dict(zip(keys, combo), psnr=both, mean=float(np.mean(list(both.values()))), clamp_only=alone,
                             clamp_only_mean=float(np.mean(list(alone.values())))))
            print("sweep:", json.dumps(rows[-1]), flush=True)
        rows.sort(key=lambda x: -x["mean"])
        best = rows[0]
        cparams = TemporalClampParams.default(**{k: best[k] for k in keys})
        result["sweep"] = {"spps": TEMPORAL_SWEEP_SPPS, "preceding": TEMPORAL_SWEEP_PRECEDING, "seed_stride": 1,
                           "grid": CLAMP_GRID, "ranked_on": "both", "best": best, "rows": rows,
                           "without_clamp": {k: dict(psnr=v, mean=float(np.mean(list(v.values())))) for k, v in baseline.items()}}
        print("sweep: best", best, flush=True)
        del held
    result["params"] = cparams.as_dict()
    result["guided_params"] = gparams.as_dict()

    table, timing = [], []
    for spp in TEMPORAL_SPPS:
        cfg = N.RenderConfig.make(W, H, spp)
        scene = N.Scene(ASSETS, cfg)
        for f in FRAMES:
            scene.setup_frame(f)
            r.upload(scene)
            raw, racc, rmom = r.render_moments(cfg, want_accum=True)
            ralb, rnd = r.render_features(cfg)
            _, single = r.denoise_guided(racc, ralb, rnd, rmom)
            base = {"spp": spp, "frame": f, "psnr_raw": psnr_half(ref_half[f], raw),
                    "psnr_guided": psnr_half(ref_half[f], single)}
            for n in TEMPORAL_PRECEDING:
                steps = frames_of(scene, cfg, sequence(f, n))
                row = dict(base, preceding=n, subframes=len(steps[-1][0]))
                for arm, (cp, k) in arms_of(cparams).items():
                    h, found, clipped = accumulate(steps, cp, k)
                    _, bgra = r.denoise_guided(h[1], h[3], h[4], h[2], gparams)
                    row[arm] = {"psnr_temporal": psnr_half(ref_half[f], tonemapped(h[1])),
                                "psnr_temporal_guided": psnr_half(ref_half[f], bgra), "found": found, "clipped": clipped}
                table.append(row)
                print(json.dumps(row), flush=True)
            if spp == TEMPORAL_SPPS[-1]:
                # the kernel is a fraction of a millisecond: the mean of 20 runs back to back
                prev, _, _ = accumulate(steps[:-1], cparams, CLAMP_BLUR_CAMERAS)
                cams, acc, mom, alb, nd = steps[-1]
                for n_cams in CLAMP_TIMED_CAMERAS:
                    use = (cams * n_cams)[:n_cams] if n_cams > 1 else [cams[len(cams) // 2]]
                    for radius in (0, 1, 2):
                        cp = TemporalClampParams.default(clamp_radius=radius)
                        cp.clamp_sigma, cp.clipped_history = cparams.clamp_sigma, cparams.clipped_history
                        _, ms, _ = timed(lambda: [r.temporal_accumulate_clamped(use, acc, mom, alb, nd, prev, cp)
                                                  for _ in range(20)][-1])
                        timing.append({"frame": f, "spp": spp, "n_cams": n_cams, "clamp_radius": radius, "ms": ms / 20})
                _, ms, _ = timed(lambda: [r.temporal_accumulate(cams[len(cams) // 2], acc, mom, alb, nd, prev, cparams.base)
                                          for _ in range(20)][-1])
                timing.append({"frame": f, "spp": spp, "kernel": "k_temporal_accumulate", "ms": ms / 20})
                print(json.dumps(timing[-10:]), flush=True)
        scene.close()
    result["table"] = table
    result["kernel_ms"] = timing
    os.makedirs(args.out, exist_ok=True)
    dump_rows_compact(result, os.path.join(args.out, "temporal_clamp_study.json"))
    print("wrote", os.path.join(args.out, "temporal_clamp_study.json"))


ADAPTIVE_BUDGETS = (64, 256, 1024)
ADAPTIVE_PASSES = 8
ADAPTIVE_SWEEP_BUDGETS = (64, 256)
ADAPTIVE_GRID = {"threshold": (0.025, 0.05, 0.1, 0.2), "dilate": (0, 1, 2)}
ADAPTIVE_REF_SPP_1024 = 4096                     # the 1024-spp budget is judged against a 4096-spp frame
ADAPTIVE_CHECK = {"width": 160, "height": 90, "budget": 64, "frame": 0, "reference_spp": 256}


def adaptive_study(args):
    """Adaptive sampling against uniform sampling of the same cost.  Per row
    (budget N, frame, threshold, dilate; passes 8, min_passes 1, the library's
    luminance_floor): the samples the adaptive render took, its active pixels
    per pass, time and PSNR, beside ptg_render at the smallest multiple of 8
    spp whose samples are at least as many (on a scene set up for that spp:
    its subframes cover the shutter).  The 1024-spp budget is judged against
    a 4096-spp frame, the others against the 1024-spp frame.  --sweep runs the
    grid over budgets 64 and 256 and ranks the rows by the smallest gain over
    uniform sampling of the four (frame, budget) cells; without it the
    library's defaults are the only row."""
    from ptlumi.adaptive import AdaptiveParams
    r = P.GpuRenderer(0)
    lib_params = AdaptiveParams.default()
    result = {"config": {"width": W, "height": H, "frames": FRAMES, "budgets": ADAPTIVE_BUDGETS, "passes": ADAPTIVE_PASSES,
                         "reference_spp": {str(n): ADAPTIVE_REF_SPP_1024 if n >= REF_SPP else REF_SPP
                                           for n in ADAPTIVE_BUDGETS}},
              "device": torch.cuda.get_device_name(0), "library_params": lib_params.as_dict()}
    npix = W * H

    def half(bgra):
        return V.downscale_half(V.bgra_to_rgb(bgra.cpu().numpy()))

    def params(threshold, dilate):
        return AdaptiveParams.default(passes=ADAPTIVE_PASSES, min_passes=1, threshold=threshold, dilate=dilate)

    # the references, and the uniform renders by (spp, frame), each on a scene set up for its spp
    ref_half = {}
    uniform = {}

    def uniform_at(spp):
        if (spp, FRAMES[0]) in uniform:
            return
        cfg = N.RenderConfig.make(W, H, spp)
        scene = N.Scene(ASSETS, cfg)
        for f in FRAMES:
            scene.setup_frame(f)
            r.upload(scene)
            (bgra, _), ms, wall = timed(lambda: r.render(cfg))
            uniform[spp, f] = (half(bgra), ms, wall)
        scene.close()

    for spp in sorted(set(result["config"]["reference_spp"].values())):
        uniform_at(spp)
        for f in FRAMES:
            ref_half[spp, f] = uniform[spp, f][0]

    def psnr(n, f, image_half):
        """validate_frame's PSNR of a downscaled image against the budget's reference."""
        return float(V.psnr(ref_half[ADAPTIVE_REF_SPP_1024 if n >= REF_SPP else REF_SPP, f], image_half))

    grid = [dict(zip(ADAPTIVE_GRID, c)) for c in itertools.product(*ADAPTIVE_GRID.values())] if args.sweep else \
        [{"threshold": lib_params.threshold, "dilate": lib_params.dilate}]
    rows, machinery = [], []
    for n in ADAPTIVE_BUDGETS:
        cfg = N.RenderConfig.make(W, H, n)
        scene = N.Scene(ASSETS, cfg)
        for f in FRAMES:
            scene.setup_frame(f)
            r.upload(scene)
            # the machinery's cost: every pixel takes every pass, against ptg_render_moments at N
            every = params(1e-30, 0)
            _, m_ms, m_wall = timed(lambda: r.render_moments(cfg, want_accum=True))
            _, a_ms, a_wall = timed(lambda: r.render_adaptive(cfg, every))
            taken = sum(r.adaptive_stats()) * (n // ADAPTIVE_PASSES)
            _, d_ms, d_wall = timed(lambda: r.render_adaptive_denoised(cfg, every))
            row = {"budget": n, "frame": f, "render_moments_ms": m_ms, "render_moments_wall_ms": m_wall,
                   "adaptive_all_passes_ms": a_ms, "adaptive_all_passes_wall_ms": a_wall,
                   "adaptive_all_passes_share_of_budget": taken / (npix * n),
                   "adaptive_all_passes_filtered_ms": d_ms, "adaptive_all_passes_filtered_wall_ms": d_wall}
            machinery.append(row)
            print(json.dumps(row), flush=True)
            for g in grid if n in ADAPTIVE_SWEEP_BUDGETS or not args.sweep else []:
                p = params(**g)
                (bgra, _, _, _), ms, wall = timed(lambda: r.render_adaptive(cfg, p))
                active = r.adaptive_stats()
                rows.append(dict(g, budget=n, frame=f, active=active, samples=sum(active) * (n // ADAPTIVE_PASSES),
                                 ms=ms, wall_ms=wall, image=half(bgra)))
        scene.close()

    def finish(row):
        """The row's PSNR and its uniform comparison."""
        n, f = row["budget"], row["frame"]
        spp = max(8, -(-row["samples"] // (8 * npix)) * 8)
        uniform_at(spp)
        u_half, u_ms, u_wall = uniform[spp, f]
        row.update(share_of_budget=row["samples"] / (npix * n), psnr=psnr(n, f, row.pop("image")), uniform_spp=spp,
                   uniform_psnr=psnr(n, f, u_half), uniform_ms=u_ms, uniform_wall_ms=u_wall)
        row["gain_db"] = row["psnr"] - row["uniform_psnr"]
        print(json.dumps(row), flush=True)

    for row in rows:
        finish(row)
    best = {"threshold": lib_params.threshold, "dilate": lib_params.dilate}
    if args.sweep:
        ranked = []
        for g in grid:
            cells = {"%d@%d" % (x["frame"], x["budget"]): x["gain_db"] for x in rows
                     if all(x[k] == v for k, v in g.items()) and x["budget"] in ADAPTIVE_SWEEP_BUDGETS}
            ranked.append(dict(g, gain_db=cells, min_gain_db=min(cells.values())))
        ranked.sort(key=lambda x: -x["min_gain_db"])
        best = {k: ranked[0][k] for k in ADAPTIVE_GRID}
        result["sweep"] = {"budgets": ADAPTIVE_SWEEP_BUDGETS, "grid": ADAPTIVE_GRID, "best": ranked[0], "rows": ranked}
        print("sweep: best", ranked[0], flush=True)
        # the best row at the budgets the sweep left out
        for n in ADAPTIVE_BUDGETS:
            if n in ADAPTIVE_SWEEP_BUDGETS:
                continue
            cfg = N.RenderConfig.make(W, H, n)
            scene = N.Scene(ASSETS, cfg)
            for f in FRAMES:
                scene.setup_frame(f)
                r.upload(scene)
                p = params(**best)
                (bgra, _, _, _), ms, wall = timed(lambda: r.render_adaptive(cfg, p))
                active = r.adaptive_stats()
                rows.append(dict(best, budget=n, frame=f, active=active, samples=sum(active) * (n // ADAPTIVE_PASSES),
                                 ms=ms, wall_ms=wall, image=half(bgra)))
                finish(rows[-1])
            scene.close()
    result["params"] = dict(lib_params.as_dict(), passes=ADAPTIVE_PASSES, min_passes=1, **best)

    # the small end-to-end check of the suite, with the best row: no downscale
    c = ADAPTIVE_CHECK
    cnp = c["width"] * c["height"]

    def check_render(spp, adaptive):
        cfg = N.RenderConfig.make(c["width"], c["height"], spp)
        scene = N.Scene(ASSETS, cfg)
        scene.setup_frame(c["frame"])
        r.upload(scene)
        bgra = r.render_adaptive(cfg, params(**best))[0] if adaptive else r.render(cfg)[0]
        r.synchronize()
        scene.close()
        return V.bgra_to_rgb(bgra.cpu().numpy())

    check_ref = check_render(c["reference_spp"], False)
    ad = check_render(c["budget"], True)
    active = r.adaptive_stats()
    spp = max(8, -(-sum(active) * (c["budget"] // ADAPTIVE_PASSES) // (8 * cnp)) * 8)
    result["check"] = dict(c, active=active, uniform_spp=spp, psnr=float(V.psnr(check_ref, ad)),
                           uniform_psnr=float(V.psnr(check_ref, check_render(spp, False))))
    result["check"]["gain_db"] = result["check"]["psnr"] - result["check"]["uniform_psnr"]
    print("check:", json.dumps(result["check"]), flush=True)

    result["machinery"] = machinery
    result["table"] = rows
    os.makedirs(args.out, exist_ok=True)
    dump_rows_compact(result, os.path.join(args.out, "adaptive_study.json"))
    print("wrote", os.path.join(args.out, "adaptive_study.json"))


FUSED_SPPS = (8, 256)


def fused_study(args):
    """ptg_render_with_features against the two-call route it replaces: per
    (spp, frame) the HIP-event times of render_moments, render_features, the
    two back to back and render_with_features, and whether all five outputs
    of the fused call had the two calls' bits."""
    r = P.GpuRenderer(0)
    result = {"config": {"width": W, "height": H, "frames": FRAMES}, "device": torch.cuda.get_device_name(0)}
    table = []
    first = True
    for spp in (SPPS if args.sweep else FUSED_SPPS):
        cfg = N.RenderConfig.make(W, H, spp)
        scene = N.Scene(ASSETS, cfg)
        for f in FRAMES:
            scene.setup_frame(f)
            r.upload(scene, include_static=first)
            first = False
            (bgra, acc, mom), moments_ms, _ = timed(lambda: r.render_moments(cfg, want_accum=True))
            (alb, nd), features_ms, _ = timed(lambda: r.render_features(cfg))
            _, both_ms, _ = timed(lambda: (r.render_moments(cfg, want_accum=True), r.render_features(cfg)))
            fused, fused_ms, _ = timed(lambda: r.render_with_features(cfg))
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                       for a, b in zip(fused, (bgra, acc, mom, alb, nd)))
            row = {"spp": spp, "frame": f, "render_moments_ms": moments_ms, "render_features_ms": features_ms,
                   "two_calls_ms": both_ms, "render_with_features_ms": fused_ms,
                   "fused_over_moments_ms": fused_ms - moments_ms, "saved_ms": both_ms - fused_ms,
                   "saved_share_of_features": (both_ms - fused_ms) / features_ms, "outputs_equal_bits": same}
            table.append(row)
            print(json.dumps(row), flush=True)
        scene.close()
    result["table"] = table
    result["all_outputs_equal_bits"] = all(row["outputs_equal_bits"] for row in table)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "fused_study.json"), "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", os.path.join(args.out, "fused_study.json"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--temporal", action="store_true")
    ap.add_argument("--temporal-clamp", action="store_true")
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_study"))
    args = ap.parse_args()
    if args.fused:
        return fused_study(args)
    if args.adaptive:
        return adaptive_study(args)
    if args.guided:
        return guided_study(args)
    if args.temporal:
        return temporal_study(args)
    if args.temporal_clamp:
        return temporal_clamp_study(args)
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
