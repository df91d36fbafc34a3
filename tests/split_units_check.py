"""Helper of tests/test_gpu_split_units.py, run as its own process: libptg.so
holds one code object per HIP unit (pt_kernels.hip, image_ops.hip,
upload.hip), and this process's first GPU work is in the image-space unit,
with no scene uploaded and nothing rendered - so no kernel of the render or
upload unit has run when k_tonemap and the denoiser's kernels are launched.
ptg_tonemap on the inputs of test_gpu_parity.test_tonemap_bit_exact against
the oracle, then ptg_denoise (1 iteration, 16x16) against its CPU
restatement.  Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ptlumi_loader  # noqa: E402,F401
from ptlumi import native as N  # noqa: E402


def tonemap_inputs():
    import numpy as np
    rng = np.random.default_rng(1)
    return np.concatenate([
        np.linspace(0, 2, 4096, dtype=np.float32)[:, None].repeat(3, 1),
        rng.exponential(0.5, (4096, 3)).astype(np.float32),
        np.array([[0, 0, 0], [1e-8, 0.0031308, 0.0031307], [1e6, 50, 3], [-1, -0.0, 2.5]], np.float32),
    ])


def main():
    import numpy as np
    from denoise_inputs import fixed_inputs
    from oracle import tonemap as oracle_tonemap
    from ptlumi.denoise import DenoiseParams, atrous_reference
    from ptlumi.renderer import GpuRenderer
    r = GpuRenderer(0)
    # the first launch of this process: k_tonemap, through host pointers
    c = tonemap_inputs()
    tonemap_equal = bool(np.array_equal(r.tonemap(c), oracle_tonemap(c)))

    import torch
    w = h = 16
    P = DenoiseParams.default(iterations=1)
    rad, alb, nd = fixed_inputs(w, h, 7 * w + h)
    want = atrous_reference(rad, alb, nd, P)
    out, _ = r.denoise(*(torch.from_numpy(a).to("cuda:0") for a in (rad, alb, nd)), P, want_bgra=False)
    r.synchronize()
    got = out.cpu().numpy()
    # equal bit patterns; two NaNs count as equal (tests/test_gpu_denoise.py)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    r.close()
    print(json.dumps({"lib": os.path.basename(N.LIB_PATH), "tonemap_equal": tonemap_equal, "tonemap_n": int(len(c)),
                      "denoise_differ": int((~same).sum()), "denoise_finite": bool(np.isfinite(got).all())}), flush=True)


if __name__ == "__main__":
    main()
