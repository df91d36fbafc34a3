"""MI355X-native path tracer (gfx950) - drop-in for the per-pixel hot path of
Kalache-abdesattar/Path-Tracing...but-on-the-LUMI-cluster.

Registered as ``ptlumi`` by ``ptlumi_loader`` (the directory name is not a
Python identifier).  Layout:

  csrc/            three HIP units over csrc/runtime.h and csrc/device/ - the
                   path tracer (pt_kernels.hip), the image-space filters
                   (image_ops.hip), the upload (upload.hip) - and the host
                   C++ scene restatement (csrc/host/) -> _build/libptg.so
  native.py        ctypes binding of include/ptg.h
  renderer.py      GpuRenderer: upload + render through the C ABI;
                   TemporalDenoiser: a frame sequence through the temporal
                   accumulation and the variance-guided filter
  denoise.py       the parameter structures and the CPU restatements of
                   ptg_denoise, ptg_denoise_guided and ptg_temporal_accumulate
                   (NumPy float32 + the C library's exp)
  adaptive.py      AdaptiveParams and the CPU restatement of ptg_render_adaptive
                   (adaptive sampling over per-sample radiance)
  distributed.py   one process per GPU: tile / frame sharding, RCCL gather
  validator.py     validator.py-equivalent PSNR check (numpy)
  assets.py        scene asset preparation (reference OBJs + substitutes)
  build.py         in-tree build of libptg.so for gfx950
"""
from . import assets, native, validator  # noqa: F401
from .native import RenderConfig, Scene, write_bmp  # noqa: F401

__all__ = ["assets", "native", "validator", "RenderConfig", "Scene", "write_bmp", "GpuRenderer", "TemporalDenoiser"]


def __getattr__(name):
    if name in ("GpuRenderer", "TemporalDenoiser"):
        from . import renderer
        return getattr(renderer, name)
    raise AttributeError(name)
