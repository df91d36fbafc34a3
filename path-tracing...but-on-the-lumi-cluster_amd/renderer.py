"""GPU renderer: the MI355X replacement of the reference's baseline_render.

``GpuRenderer`` owns one ``ptg_context`` (one GPU).  The reference drives its
hot path as

    load_scene(); setup_animation_frame(s, f); baseline_render(s, image)
    (main.cc:67, :82, :88)

and the same flow here is

    scene = Scene(assets, cfg); scene.setup_frame(f)
    r = GpuRenderer(device); r.upload(scene); img = r.render(cfg)

Everything below the C ABI runs in HIP kernels; this class only moves
pointers.  Device outputs are torch tensors (torch is used for device memory,
streams and torch.distributed only).  There is no CPU fallback: without a
gfx950 device the constructor raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native as N


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _span(cfg, rect=None, samples=None):
    """(x0, y0, w, h, j0, j1): `rect` and the sample range `samples` with
    their defaults, the whole image and every sample of `cfg`."""
    x0, y0, w, h = rect if rect is not None else (0, 0, cfg.width, cfg.height)
    j0, j1 = samples if samples is not None else (0, cfg.samples_per_pixel)
    return x0, y0, w, h, j0, j1


def _planes(device, h, w, *want):
    """Empty planes of an [h, w] image on `device` (a torch.device or a GPU
    ordinal), one per entry of `want` and None where the entry is false: the
    first is bgra, uint8 [h, w, 4], every other one float32 [h, w, 4]."""
    import torch
    dev = device if isinstance(device, torch.device) else torch.device("cuda", device)
    return tuple(torch.empty((h, w, 4), dtype=torch.float32 if k else torch.uint8, device=dev) if on else None
                 for k, on in enumerate(want))


class GpuRenderer:
    def __init__(self, device: int = 0, stream=None):
        import torch  # noqa: F401  (device memory + streams)
        self._ctx = C.c_void_p()
        N.check(N.lib().ptg_context_create(device, C.byref(self._ctx)), "ptg_context_create")
        self.device = device
        self.scene_uploaded = False
        if stream is not None:
            self.set_stream(stream)

    # -- streams ---------------------------------------------------------
    def set_stream(self, stream):
        """Launch on a torch.cuda.Stream (or raw hipStream_t int)."""
        handle = getattr(stream, "cuda_stream", stream)
        N.check(N.lib().ptg_context_set_stream(self._ctx, C.c_void_p(handle)), "ptg_context_set_stream")

    def synchronize(self):
        N.check(N.lib().ptg_synchronize(self._ctx), "ptg_synchronize")

    # -- uploads ---------------------------------------------------------
    def upload(self, scene: N.Scene, include_static=None):
        """upload_scene (once) + upload_frame (every frame) from a host Scene."""
        if include_static is None:
            include_static = not self.scene_uploaded
        N.check(N.lib().ptg_upload_from_scene(self._ctx, scene.handle, 1 if include_static else 0),
                "ptg_upload_from_scene")
        self.scene_uploaded = True

    def upload_arrays(self, arrays: dict, include_static=True, include_frame=True):
        """Upload reference-layout numpy arrays (the keys of Scene.view()):
        ptg_upload_scene (include_static) and/or ptg_upload_frame (include_frame)."""
        L = N.lib()
        a = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in arrays.items()}
        sn = int(a["static_node_count"])
        if include_static:
            N.check(L.ptg_upload_scene(self._ctx, a["nodes"].ctypes.data, a["links"].ctypes.data, sn,
                                       a["indices"].ctypes.data, a["indices"].size, a["pos"].ctypes.data,
                                       a["normal"].ctypes.data, a["albedo"].ctypes.data, a["material"].ctypes.data,
                                       a["pos"].shape[0]), "ptg_upload_scene")
        if not include_frame:
            self.scene_uploaded = self.scene_uploaded or include_static
            return
        nodes = a["nodes"][sn:]
        links = a["links"][8 * sn:]
        N.check(L.ptg_upload_frame(self._ctx, a["subframes"].ctypes.data, a["subframes"].size,
                                   a["instances"].ctypes.data, a["instances"].size,
                                   np.ascontiguousarray(nodes).ctypes.data, np.ascontiguousarray(links).ctypes.data,
                                   sn, nodes.size), "ptg_upload_frame")
        self.scene_uploaded = True

    # -- rendering -------------------------------------------------------
    def render(self, cfg: N.RenderConfig, rect=None, samples=None, out_bgra=None, out_accum=None,
               want_accum=False):
        """baseline_render over `rect` = (x0, y0, w, h) (default: the whole
        image) and sample range `samples` = (begin, end) (default: all).
        Returns (bgra uint8 [h, w, 4], accum float32 [h, w, 4] or None) as
        torch tensors on this GPU.  Asynchronous on the context stream."""
        x0, y0, w, h, j0, j1 = _span(cfg, rect, samples)
        bgra, accum = _planes(self.device, h, w, out_bgra is None, want_accum and out_accum is None)
        out_bgra = out_bgra if out_bgra is not None else bgra
        out_accum = out_accum if out_accum is not None else accum
        N.check(N.lib().ptg_render(self._ctx, C.byref(cfg), x0, y0, w, h, j0, j1, _ptr(out_accum), _ptr(out_bgra)),
                "ptg_render")
        return out_bgra, out_accum

    def render_tiles(self, cfg: N.RenderConfig, tile_w, tile_h, first, stride, count, out_bgra=None,
                     out_accum=None):
        """Render an interleaved tile set densely (multi-GPU sharding unit)."""
        import torch
        dev = torch.device("cuda", self.device)
        n = count * tile_w * tile_h
        if out_bgra is None:
            out_bgra = torch.empty((n, 4), dtype=torch.uint8, device=dev)
        N.check(N.lib().ptg_render_tiles(self._ctx, C.byref(cfg), tile_w, tile_h, first, stride, count,
                                         _ptr(out_accum), _ptr(out_bgra)), "ptg_render_tiles")
        return out_bgra, out_accum

    def scatter_tiles(self, cfg, tile_w, tile_h, first, stride, count, tiles_bgra, image_bgra):
        N.check(N.lib().ptg_scatter_tiles(self._ctx, C.byref(cfg), tile_w, tile_h, first, stride, count,
                                          _ptr(tiles_bgra), _ptr(image_bgra)), "ptg_scatter_tiles")

    def render_tiles_packed(self, cfg: N.RenderConfig, tile_w, tile_h, first, stride, count, pack_tiles, out=None):
        """render_with_features over an interleaved tile set, all five planes
        in one tile pack sized for `pack_tiles` tiles (ptg_render_tiles_packed;
        distributed.tile_pack_layout names the planes' offsets): a uint8
        device tensor of ptg_tile_pack_bytes bytes, every byte that is no
        image pixel 0.  `out` may be such a tensor (one row of a gathered
        buffer).  Asynchronous."""
        import torch
        nbytes = N.lib().ptg_tile_pack_bytes(tile_w, tile_h, pack_tiles)
        if out is None:
            out = torch.empty((nbytes,), dtype=torch.uint8, device=torch.device("cuda", self.device))
        assert out.dtype == torch.uint8 and out.numel() == nbytes and out.is_contiguous()
        N.check(N.lib().ptg_render_tiles_packed(self._ctx, C.byref(cfg), tile_w, tile_h, first, stride, count, pack_tiles,
                                                _ptr(out)), "ptg_render_tiles_packed")
        return out

    def assemble_tile_packs(self, cfg: N.RenderConfig, tile_w, tile_h, world, pack_tiles, packs):
        """The frame from the gathered packs of a `world`-rank tile shard
        (`packs`: a contiguous uint8 device tensor, world packs back to back)
        in one launch (ptg_assemble_tile_packs): (bgra, accum, moments,
        albedo+coverage, normal+depth), render_with_features' order and
        shapes.  Asynchronous."""
        import torch
        assert packs.dtype == torch.uint8 and packs.is_contiguous()
        assert packs.numel() == world * N.lib().ptg_tile_pack_bytes(tile_w, tile_h, pack_tiles)
        bgra, accum, moments, albedo, normal_depth = _planes(packs.device, cfg.height, cfg.width, *[True] * 5)
        N.check(N.lib().ptg_assemble_tile_packs(self._ctx, C.byref(cfg), tile_w, tile_h, world, pack_tiles, _ptr(packs),
                                                _ptr(accum), _ptr(bgra), _ptr(moments), _ptr(albedo), _ptr(normal_depth)),
                "ptg_assemble_tile_packs")
        return bgra, accum, moments, albedo, normal_depth

    # -- per-sample / per-ray entry points (parity) -------------------------
    def path_trace_samples(self, cfg, xy: np.ndarray, sample_index: np.ndarray) -> np.ndarray:
        xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
        js = np.ascontiguousarray(sample_index, dtype=np.int32).reshape(-1)
        out = np.zeros((len(js), 4), np.float32)
        N.check(N.lib().ptg_path_trace_samples(self._ctx, C.byref(cfg), len(js), xy.ctypes.data, js.ctypes.data,
                                               out.ctypes.data), "ptg_path_trace_samples")
        return out

    def trace_rays(self, subframe: int, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        hits = np.zeros((len(rays), 8), np.uint32)
        N.check(N.lib().ptg_trace_rays(self._ctx, subframe, len(rays), rays.ctypes.data, hits.ctypes.data),
                "ptg_trace_rays")
        return hits

    def walk_rays(self, subframe: int, rays: np.ndarray, round: int = 0, grid_blocks: int = 0, counted: bool = False):
        """The render's walk kernels over `rays` (float32 [n, 6]: origin,
        direction) as bounce round `round`'s queue (ptg_walk_rays):
        (hits uint32 [n, 8] in trace_rays' layout, stats uint64 [2, 4] of a
        counted run or None)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        hits = np.zeros((len(rays), 8), np.uint32)
        stats = np.zeros((2, 4), np.uint64)
        N.check(N.lib().ptg_walk_rays(self._ctx, subframe, round, grid_blocks, int(bool(counted)), len(rays),
                                      rays.ctypes.data, hits.ctypes.data, stats.ctypes.data), "ptg_walk_rays")
        return hits, (stats if counted else None)

    def camera_rays(self, cfg, xy: np.ndarray, sample_index: np.ndarray):
        """The first ray of each (pixel, sample) pair (ptg_camera_rays):
        (rays float32 [n, 8] in trace_rays' layout, subframe uint32 [n])."""
        xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
        js = np.ascontiguousarray(sample_index, dtype=np.int32).reshape(-1)
        rays = np.zeros((len(js), 8), np.float32)
        sub = np.zeros(len(js), np.uint32)
        N.check(N.lib().ptg_camera_rays(self._ctx, C.byref(cfg), len(js), xy.ctypes.data, js.ctypes.data,
                                        rays.ctypes.data, sub.ctypes.data), "ptg_camera_rays")
        return rays, sub

    # -- first-hit features and the denoiser ----------------------------------
    def render_features(self, cfg: N.RenderConfig, rect=None, samples=None):
        """First-hit feature buffers over `rect` and sample range `samples`
        (defaults as render()): (albedo+coverage, normal+depth), two float32
        [h, w, 4] torch tensors on this GPU.  Asynchronous."""
        x0, y0, w, h, j0, j1 = _span(cfg, rect, samples)
        _, albedo, normal_depth = _planes(self.device, h, w, False, True, True)
        N.check(N.lib().ptg_render_features(self._ctx, C.byref(cfg), x0, y0, w, h, j0, j1, _ptr(albedo),
                                            _ptr(normal_depth)), "ptg_render_features")
        return albedo, normal_depth

    def _denoise(self, entry, params, inputs, want_bgra, out_radiance):
        """ptg_denoise or ptg_denoise_guided (`entry`) over `inputs`, device
        float32 [h, w, 4] tensors with the radiance first."""
        import torch
        h, w = inputs[0].shape[:2]
        for t in inputs:
            assert t.dtype == torch.float32 and tuple(t.shape) == (h, w, 4) and t.is_contiguous()
        if out_radiance is None:
            out_radiance = torch.empty_like(inputs[0])
        bgra = torch.empty((h, w, 4), dtype=torch.uint8, device=inputs[0].device) if want_bgra else None
        N.check(getattr(N.lib(), entry)(self._ctx, w, h, C.byref(params), *map(_ptr, inputs), _ptr(out_radiance), _ptr(bgra)),
                entry)
        return out_radiance, bgra

    def denoise(self, radiance, albedo, normal_depth, params=None, want_bgra=True, out_radiance=None):
        """ptg_denoise over device float32 [h, w, 4] tensors: (denoised
        radiance, bgra uint8 [h, w, 4] or None).  `out_radiance` may be
        `radiance` itself.  Asynchronous."""
        from .denoise import DenoiseParams
        p = params if params is not None else DenoiseParams.default()
        return self._denoise("ptg_denoise", p, (radiance, albedo, normal_depth), want_bgra, out_radiance)

    def render_with_features(self, cfg: N.RenderConfig, rect=None, samples=None, want_moments=True):
        """render_moments (without `want_moments`: render) and render_features
        in one pass (ptg_render_with_features): (bgra, accum, moments or None,
        albedo+coverage, normal+depth), each with the bits the separate calls
        give.  On the wavefront pipeline the features come from the render's
        own primary rays, so no second walk is made.  Asynchronous."""
        x0, y0, w, h, j0, j1 = _span(cfg, rect, samples)
        bgra, accum, moments, albedo, normal_depth = _planes(self.device, h, w, True, True, want_moments, True, True)
        N.check(N.lib().ptg_render_with_features(self._ctx, C.byref(cfg), x0, y0, w, h, j0, j1, _ptr(accum), _ptr(bgra),
                                                 _ptr(moments), _ptr(albedo), _ptr(normal_depth)),
                "ptg_render_with_features")
        return bgra, accum, moments, albedo, normal_depth

    def render_denoised(self, cfg: N.RenderConfig, params=None, fused=True):
        """render + render_features + denoise of the whole image: (bgra,
        denoised radiance).  `fused` (the default) takes the radiance and the
        features from one render_with_features pass; fused=False makes the
        two calls: the same bits.  Asynchronous."""
        if fused:
            _, acc, _, albedo, normal_depth = self.render_with_features(cfg, want_moments=False)
        else:
            _, acc = self.render(cfg, want_accum=True)
            albedo, normal_depth = self.render_features(cfg)
        out, bgra = self.denoise(acc, albedo, normal_depth, params, want_bgra=True, out_radiance=acc)
        return bgra, out

    # -- sample moments and the variance-guided denoiser ----------------------
    def render_moments(self, cfg: N.RenderConfig, rect=None, samples=None, want_accum=False):
        """render() that also keeps the samples' luminance moments
        (ptg_render_moments): (bgra, accum or None, moments float32 [h, w, 4] =
        (mean, second moment, variance of the mean, finite samples)).  The
        moments are normalised by the finite samples of the range rendered.
        Asynchronous."""
        x0, y0, w, h, j0, j1 = _span(cfg, rect, samples)
        bgra, accum, moments = _planes(self.device, h, w, True, want_accum, True)
        N.check(N.lib().ptg_render_moments(self._ctx, C.byref(cfg), x0, y0, w, h, j0, j1, _ptr(accum), _ptr(bgra),
                                           _ptr(moments)), "ptg_render_moments")
        return bgra, accum, moments

    def denoise_guided(self, radiance, albedo, normal_depth, moments, params=None, want_bgra=True, out_radiance=None):
        """ptg_denoise_guided over device float32 [h, w, 4] tensors: (denoised
        radiance, bgra uint8 [h, w, 4] or None).  `out_radiance` may be
        `radiance` itself.  Asynchronous."""
        from .denoise import DenoiseGuidedParams
        p = params if params is not None else DenoiseGuidedParams.default()
        return self._denoise("ptg_denoise_guided", p, (radiance, albedo, normal_depth, moments), want_bgra, out_radiance)

    def render_denoised_guided(self, cfg: N.RenderConfig, params=None, fused=True):
        """render_moments + render_features + denoise_guided of the whole
        image: (bgra, denoised radiance).  `fused` as for render_denoised.
        Asynchronous."""
        if fused:
            _, acc, moments, albedo, normal_depth = self.render_with_features(cfg)
        else:
            _, acc, moments = self.render_moments(cfg, want_accum=True)
            albedo, normal_depth = self.render_features(cfg)
        out, bgra = self.denoise_guided(acc, albedo, normal_depth, moments, params, want_bgra=True, out_radiance=acc)
        return bgra, out

    # -- adaptive sampling ---------------------------------------------------
    def render_adaptive(self, cfg: N.RenderConfig, params=None, rect=None):
        """ptg_render_adaptive over `rect` (default: the whole image) with
        cfg.samples_per_pixel as the budget: (bgra, accum, moments float32
        [h, w, 4] in render_moments' layout, samples [h, w]: the samples each
        pixel took, the library's uint32 in an int32 tensor).  The call waits for the GPU once per selection pass;
        the outputs are queued asynchronously."""
        import torch
        from .adaptive import AdaptiveParams
        p = params if params is not None else AdaptiveParams.default()
        x0, y0, w, h, _, _ = _span(cfg, rect)
        bgra, accum, moments = _planes(self.device, h, w, True, True, True)
        samples = torch.empty((h, w), dtype=torch.int32, device=bgra.device)
        N.check(N.lib().ptg_render_adaptive(self._ctx, C.byref(cfg), x0, y0, w, h, C.byref(p), _ptr(accum), _ptr(bgra),
                                            _ptr(moments), _ptr(samples)), "ptg_render_adaptive")
        return bgra, accum, moments, samples

    def adaptive_stats(self):
        """The last render_adaptive: the active pixel count of every pass it
        ran (ptg_last_adaptive_stats); a pass is budget / passes samples."""
        n = C.c_uint32()
        active = np.zeros(16, np.uint64)
        N.check(N.lib().ptg_last_adaptive_stats(self._ctx, C.byref(n), active.ctypes.data), "ptg_last_adaptive_stats")
        return [int(a) for a in active[:n.value]]

    def render_adaptive_denoised(self, cfg: N.RenderConfig, params=None, guided_params=None):
        """render_adaptive + render_features + denoise_guided of the whole
        image: (bgra, denoised radiance).  The filter reads the moments of the
        samples each pixel took."""
        _, acc, moments, _ = self.render_adaptive(cfg, params)
        albedo, normal_depth = self.render_features(cfg)
        out, bgra = self.denoise_guided(acc, albedo, normal_depth, moments, guided_params, want_bgra=True, out_radiance=acc)
        return bgra, out

    # -- progressive rendering -------------------------------------------------
    def render_progressive(self, cfg: N.RenderConfig, steps, rect=None, moments=True, features=True, sample_begin=0):
        """A generator over one ``Accumulator``: for each sample end of the
        increasing list `steps` it adds the samples up to there and yields
        (samples_done, accumulator); ``accumulator.resolve()`` then gives the
        image so far, and after the last step the bits of the one-shot
        render.  The caller may stop iterating at any step."""
        acc = Accumulator(self, cfg, rect=rect, moments=moments, features=features, sample_begin=sample_begin)
        for end in steps:
            acc.add(end)
            yield acc.samples_done, acc

    # -- temporal accumulation -------------------------------------------------
    def _temporal(self, entry, p, cams, radiance, moments, albedo, normal_depth, history, want_bgra, out_radiance,
                  out_moments, flags=()):
        """The two temporal entries' shared half: the images checked, the
        outputs allocated, `entry` called with its own camera arguments
        `cams` and, behind bgra, its own trailing `flags`."""
        import torch
        images = (radiance, moments, albedo, normal_depth) + (tuple(history[1:]) if history is not None else ())
        h, w = radiance.shape[:2]
        for t in images:
            assert t.dtype == torch.float32 and tuple(t.shape) == (h, w, 4) and t.is_contiguous()
        hc = N.Camera.of(history[0]) if history is not None else None
        if out_radiance is None:
            out_radiance = torch.empty_like(radiance)
        if out_moments is None:
            out_moments = torch.empty_like(moments)
        bgra = torch.empty((h, w, 4), dtype=torch.uint8, device=radiance.device) if want_bgra else None
        hist = images[4:] if history is not None else (None,) * 4
        N.check(getattr(N.lib(), entry)(self._ctx, w, h, C.byref(p), *cams, C.byref(hc) if hc is not None else None,
                                        *map(_ptr, images[:4]), *map(_ptr, hist), _ptr(out_radiance), _ptr(out_moments),
                                        _ptr(bgra), *map(_ptr, flags)), entry)
        return out_radiance, out_moments, bgra

    def temporal_accumulate(self, cam, radiance, moments, albedo, normal_depth, history=None, params=None,
                            want_bgra=False, out_radiance=None, out_moments=None):
        """ptg_temporal_accumulate over device float32 [h, w, 4] tensors:
        (accumulated radiance, accumulated moments, bgra uint8 [h, w, 4] or
        None).  `cam` is this frame's camera (a native.Camera or a
        CAMERA_DTYPE record); `history` is None (first frame) or (hist_cam,
        hist_radiance, hist_moments, hist_albedo, hist_normal_depth): the
        previous frame's camera, the previous call's two outputs and the
        previous frame's guides.  `out_radiance` / `out_moments` may be
        `radiance` / `moments` themselves, never a history tensor.
        Asynchronous."""
        from .denoise import TemporalParams
        p = params if params is not None else TemporalParams.default()
        c = N.Camera.of(cam)
        return self._temporal("ptg_temporal_accumulate", p, (C.byref(c),), radiance, moments, albedo, normal_depth, history,
                              want_bgra, out_radiance, out_moments)

    def temporal_accumulate_clamped(self, cams, radiance, moments, albedo, normal_depth, history=None, params=None,
                                    want_bgra=False, out_radiance=None, out_moments=None, want_flags=False):
        """ptg_temporal_accumulate_clamped: temporal_accumulate through the
        list `cams` of this frame's cameras (1 .. 512 native.Camera or
        CAMERA_DTYPE records, e.g. a motion-blurred frame's subframe cameras),
        the history clamped to the frame's local colour box as `params` (a
        denoise.TemporalClampParams) says.  Returns (accumulated radiance,
        accumulated moments, bgra or None), and with `want_flags` a fourth
        value: the uint8 [h, w] device tensor of the pixels' flags, written
        on the context's stream like the images (``split_flags`` gives the
        found and the clipped mask).  `out_moments` may be `moments`;
        `out_radiance` may be `radiance` only with clamp_radius 0.
        Asynchronous."""
        import torch
        from .denoise import TemporalClampParams
        p = params if params is not None else TemporalClampParams.default()
        cams = [cams[k] for k in range(len(cams))] if isinstance(cams, np.ndarray) else list(cams)
        c = (N.Camera * max(len(cams), 1))(*(N.Camera.of(cam) for cam in cams))
        flags = torch.empty(radiance.shape[:2], dtype=torch.uint8, device=radiance.device) if want_flags else None
        out = self._temporal("ptg_temporal_accumulate_clamped", p, (len(cams), c), radiance, moments, albedo, normal_depth,
                             history, want_bgra, out_radiance, out_moments, (flags,))
        return out + (flags,) if want_flags else out

    @staticmethod
    def split_flags(flags):
        """(found, clipped) bool masks of temporal_accumulate_clamped's flags
        (a tensor, after a synchronize, or its numpy copy): bit 0 the pixel
        found history, bit 1 its history was clipped."""
        return (flags & 1) != 0, (flags & 2) != 0

    def tonemap_device(self, colors, out_bgra):
        """tonemap_pixel over a device float32 [..., 4] tensor into a device
        uint8 [..., 4] tensor (ptg_tonemap_device; asynchronous)."""
        n = colors.numel() // 4
        assert out_bgra.numel() == 4 * n
        N.check(N.lib().ptg_tonemap_device(self._ctx, n, _ptr(colors), _ptr(out_bgra)), "ptg_tonemap_device")
        return out_bgra

    def tonemap(self, colors: np.ndarray) -> np.ndarray:
        c = np.zeros((colors.shape[0], 4), np.float32)
        c[:, :colors.shape[1]] = colors[:, :4] if colors.shape[1] >= 4 else colors
        c = np.ascontiguousarray(c)
        out = np.zeros((len(c), 4), np.uint8)
        N.check(N.lib().ptg_tonemap(self._ctx, len(c), c.ctypes.data, out.ctypes.data), "ptg_tonemap")
        return out

    def enable_timing(self, on=True):
        N.check(N.lib().ptg_timing_enable(self._ctx, 1 if on else 0), "ptg_timing_enable")

    def last_timing(self):
        """(summed path-kernel device ms, launch count) since timing was enabled or last read."""
        ms, n = C.c_double(), C.c_uint32()
        N.check(N.lib().ptg_last_timing(self._ctx, C.byref(ms), C.byref(n)), "ptg_last_timing")
        return ms.value, n.value

    KINDS = ("megakernel", "extend", "shadow", "shade", "camera", "accumulate", "sky", "classify")

    def kernel_times(self):
        """{kind: (device ms, launches)} summed over the launches recorded since
        timing was enabled or last read (waits for them; clears the record)."""
        ms = np.zeros(8, np.float64)
        n = np.zeros(8, np.uint32)
        N.check(N.lib().ptg_last_kernel_times(self._ctx, ms.ctypes.data, n.ctypes.data), "ptg_last_kernel_times")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.KINDS)}

    def kernel_busy(self):
        """{kind: (busy ms, summed ms, launches)}: busy = the union of the
        recorded launches' device intervals (overlapping launches of one kind
        counted once); waits for them and clears the record."""
        busy = np.zeros(8, np.float64)
        ms = np.zeros(8, np.float64)
        n = np.zeros(8, np.uint32)
        N.check(N.lib().ptg_last_kernel_busy(self._ctx, busy.ctypes.data, ms.ctypes.data, n.ctypes.data),
                "ptg_last_kernel_busy")
        return {k: (float(busy[i]), float(ms[i]), int(n[i])) for i, k in enumerate(self.KINDS)}

    def kernel_counters(self):
        """{kind: counters[8]} of the last render call (counting enabled)."""
        out = np.zeros((6, 8), np.uint64)
        N.check(N.lib().ptg_last_kernel_counters(self._ctx, out.ctypes.data), "ptg_last_kernel_counters")
        return {k: out[i] for i, k in enumerate(self.KINDS[:6])}

    WALK_STATS = ("node_phases", "node_lanes", "leaf_phases", "leaf_lanes", "refills", "refill_lanes", "iterations",
                  "active_lanes")

    def walk_stats(self):
        """{"extend"|"shadow": {stat: count}} of the last counted render: the
        walks' phases that loaded records and the lanes they served
        (ptg_last_walk_stats)."""
        out = np.zeros((2, 8), np.uint64)
        N.check(N.lib().ptg_last_walk_stats(self._ctx, out.ctypes.data), "ptg_last_walk_stats")
        return {k: {s: int(out[i, j]) for j, s in enumerate(self.WALK_STATS)} for i, k in enumerate(("extend", "shadow"))}

    def set_hbm_share(self, percent):
        """Cap the wavefront path state at `percent` of HBM per chunk pipeline
        (default 35); identical bits at any share."""
        N.check(N.lib().ptg_set_hbm_share(self._ctx, int(percent)), "ptg_set_hbm_share")

    def set_chunk_paths(self, log2_paths):
        """At most 2^log2_paths live paths per sample chunk and pipeline
        (16-28, default 27); identical bits at any size."""
        N.check(N.lib().ptg_set_chunk_paths(self._ctx, int(log2_paths)), "ptg_set_chunk_paths")

    def set_pipeline(self, name):
        """'wavefront' (default) or 'megakernel' - bit-identical results."""
        N.check(N.lib().ptg_set_pipeline(self._ctx, {"wavefront": 0, "megakernel": 1}[name]), "ptg_set_pipeline")

    def redo_stats(self):
        """Counting renders: paths the certified shading passes handed to the
        exact (glibc-algorithm) pass - {"surface", "sky", "sites": {site: n}}
        (ptg_last_redo_stats)."""
        out = np.zeros(9, np.uint64)
        N.check(N.lib().ptg_last_redo_stats(self._ctx, out.ctypes.data), "ptg_last_redo_stats")
        names = ("acc_exp", "exp_times", "add_mul_pow", "div_mul_pow", "times_cos", "times_sin",
                 "times_one_minus_div_pow")
        return {"surface": int(out[0]), "sky": int(out[1]), "sites": {n: int(out[2 + k]) for k, n in enumerate(names)}}

    def selftest(self):
        """ptg_arith_selftest: mask of the failed arithmetic known-answer checks (0 = all
        passed) of the library's own build on this device against this host's libm."""
        m = N.lib().ptg_arith_selftest(self._ctx)
        if m < 0:
            N.check(m, "ptg_arith_selftest")
        return int(m)

    def set_concurrency(self, level):
        """0: one stream; 1: sky/shadow kernels on a second stream; 2 (default):
        also two sample chunks in flight.  Identical bits at every level."""
        N.check(N.lib().ptg_set_concurrency(self._ctx, int(level)), "ptg_set_concurrency")

    def enable_counters(self, on=True):
        N.check(N.lib().ptg_counters_enable(self._ctx, 1 if on else 0), "ptg_counters_enable")

    def counters(self):
        out = np.zeros(8, np.uint64)
        N.check(N.lib().ptg_last_counters(self._ctx, out.ctypes.data), "ptg_last_counters")
        return out

    def close(self):
        if self._ctx:
            N.lib().ptg_context_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Accumulator:
    """A resumable render of one frame (ptg_accum_*): the running per-pixel
    sums as a tensor this object owns, ``state`` (float32 [planes, h, w, 4]
    on the renderer's GPU, ptg.h's state layout: the radiance sums, then with
    `moments` the plane (s1, s2, n as bits, 0), then with `features` the
    albedo + coverage and the normal + depth sums).

    ``add(sample_end)`` traces the samples up to `sample_end` into it,
    ``resolve()`` gives the image of the samples so far and leaves the state
    alone, ``save`` / ``load`` keep it in a file.  However the samples are
    split into adds, and through a save and a load into another renderer or
    process, ``resolve()`` gives the bits of
    ``render_with_features(cfg, rect, (sample_begin, samples_done))``.  The
    renderer must have the same scene and frame uploaded at every add: that
    is the caller's contract, nothing checks it."""

    def __init__(self, renderer: GpuRenderer, cfg: N.RenderConfig, rect=None, moments=True, features=True, sample_begin=0,
                 _restore=None):
        import torch
        self.renderer = renderer
        dev = torch.device("cuda", renderer.device)
        if _restore is not None:            # Accumulator.load: the header and the planes of a checkpoint
            self.header, planes = _restore
            self.state = torch.from_numpy(planes.view(np.float32)).to(dev)
            return
        x0, y0, w, h = rect if rect is not None else (0, 0, cfg.width, cfg.height)
        flags = (N.ACCUM_MOMENTS if moments else 0) | (N.ACCUM_FEATURES if features else 0)
        self.header = N.Accum()
        self.state = torch.empty((N.accum_plane_count(flags), h, w, 4), dtype=torch.float32, device=dev)
        N.check(N.lib().ptg_accum_begin(renderer._ctx, C.byref(cfg), x0, y0, w, h, flags, sample_begin,
                                        C.byref(self.header), _ptr(self.state)), "ptg_accum_begin")

    @property
    def cfg(self):
        return self.header.cfg

    @property
    def rect(self):
        return (self.header.x0, self.header.y0, self.header.w, self.header.h)

    @property
    def moments(self):
        return bool(self.header.flags & N.ACCUM_MOMENTS)

    @property
    def features(self):
        return bool(self.header.flags & N.ACCUM_FEATURES)

    @property
    def sample_begin(self):
        return self.header.sample_begin

    @property
    def samples_done(self):
        """The sample index the state has reached: it holds [sample_begin, samples_done)."""
        return self.header.sample_next

    def add(self, sample_end):
        """Trace samples [samples_done, sample_end) into the state (ptg_accum_add).  Asynchronous."""
        N.check(N.lib().ptg_accum_add(self.renderer._ctx, C.byref(self.header), _ptr(self.state), int(sample_end)),
                "ptg_accum_add")
        return self

    def resolve(self, by_samples=False):
        """(bgra, accum, moments, albedo+coverage, normal+depth) of the samples
        so far, the order of render_with_features, with None for what the
        flags exclude.  by_samples=False divides by cfg.samples_per_pixel (the
        bits of the one-shot render of the same sample range), by_samples=True
        by the samples taken (a preview at the final brightness).  The state
        is not changed.  Asynchronous."""
        _, _, w, h = self.rect
        bgra, accum, moments, albedo, normal_depth = _planes(self.state.device, h, w, True, True, self.moments,
                                                             self.features, self.features)
        N.check(N.lib().ptg_accum_resolve(self.renderer._ctx, C.byref(self.header), _ptr(self.state), 1 if by_samples else 0,
                                          _ptr(accum), _ptr(bgra), _ptr(moments), _ptr(albedo), _ptr(normal_depth)),
                "ptg_accum_resolve")
        return bgra, accum, moments, albedo, normal_depth

    def save(self, path):
        """The checkpoint: one .npz with the 16 header words and the planes as
        uint32 [planes, h, w, 4] (native.accum_save).  Waits for the adds queued so far."""
        self.renderer.synchronize()
        N.accum_save(path, self.header, self.state.cpu().numpy())

    @classmethod
    def load(cls, renderer: GpuRenderer, path):
        """An accumulator on `renderer` continuing save's file; ValueError on
        a file that is no checkpoint (native.accum_unpack)."""
        return cls(renderer, None, _restore=N.accum_load(path))


class TemporalDenoiser:
    """A frame sequence through the temporal accumulation and the
    variance-guided filter.  ``step(scene)`` takes a host Scene set to the next
    frame and does, in order: upload, render_moments, render_features,
    temporal_accumulate against the state kept from the previous step,
    denoise_guided of the accumulated radiance with the accumulated moments;
    it returns (bgra, denoised radiance).  The camera of the reprojection is
    that of subframe ``subframe_count // 2``, the middle of the frame's
    motion blur.  Kept for the next step: the accumulated radiance and
    moments, unfiltered (the filter runs on the output for display only, so
    the history carries no spatial blur), this frame's guides and that
    camera.  ``reset()`` drops them: the next step is a first frame.

    ``seed_stride``: path_trace_pixel seeds a sample with (x, y,
    sample_index, student_id) and not with the frame, so two frames draw the
    same random numbers per pixel and their noise is correlated wherever the
    camera barely moves; accumulating such frames gains little and the
    accumulated variance understates what is left.  Step k of the sequence
    (counted from the construction or the last reset) therefore renders with
    ``student_id + k * seed_stride`` in uint32 arithmetic; frame 0 of a
    sequence has the reference's bits either way, and ``seed_stride=0`` keeps
    the reference's seeds on every frame.

    ``adaptive_params``: an ``adaptive.AdaptiveParams`` makes the step render
    with render_adaptive (cfg.samples_per_pixel is then the budget) instead
    of render_moments; the accumulation and the filter take its moments,
    whose sample count varies per pixel, as they are.  None (the default)
    renders with render_moments.

    ``fused`` (default True): a step that renders with render_moments takes
    the moments and the features from one render_with_features pass; False
    makes the two calls, render_moments then render_features: the same bits.
    An adaptive step always makes two calls (its pixels take different sample
    counts, the features every sample).

    ``clamp_params`` / ``blur_cameras``: with both at their defaults (None, 1)
    the step accumulates with temporal_accumulate, as above.  A
    ``denoise.TemporalClampParams`` as ``clamp_params`` makes it call
    temporal_accumulate_clamped with them instead (its ``base`` is then the
    accumulation's parameters, and ``temporal_params`` must be None); the
    radiance is then not accumulated in place, since the clamp reads this
    frame's neighbours.  ``blur_cameras = K > 1`` passes min(K, S) of the
    frame's S subframe cameras, evenly spaced (subframe
    ((2 k + 1) S) // (2 min(K, S)) for k = 0 ..), so that the history is
    gathered along the frame's motion blur; without ``clamp_params`` the clamp
    is then off (clamp_radius 0).  The history's camera stays the previous
    frame's middle subframe camera."""

    def __init__(self, renderer: GpuRenderer, cfg: N.RenderConfig, temporal_params=None, guided_params=None,
                 seed_stride=1, adaptive_params=None, clamp_params=None, blur_cameras=1, fused=True):
        if clamp_params is not None and temporal_params is not None:
            raise ValueError("clamp_params.base holds the accumulation's parameters: pass no temporal_params beside it")
        if int(blur_cameras) < 1:
            raise ValueError("blur_cameras must be at least 1")
        self.renderer = renderer
        self.cfg = cfg
        self.temporal_params = temporal_params
        self.guided_params = guided_params
        self.adaptive_params = adaptive_params
        self.clamp_params = clamp_params
        self.blur_cameras = int(blur_cameras)
        self.fused = bool(fused)
        self.seed_stride = int(seed_stride)
        self.reset()

    def reset(self):
        self.history = None                # (camera, radiance, moments, albedo, normal_depth) of the last step
        self.frames = 0

    def frame_config(self):
        """The configuration the next step renders with."""
        c = self.cfg
        return N.RenderConfig(c.width, c.height, c.samples_per_pixel, c.max_bounces,
                              (c.student_id + self.frames * self.seed_stride) & 0xFFFFFFFF,
                              c.samples_per_motion_blur_step)

    def blur_subframes(self, count):
        """The subframes whose cameras a step passes, of a frame with `count`:
        min(blur_cameras, count) evenly spaced; one is the middle subframe."""
        k = min(self.blur_cameras, count)
        return [((2 * j + 1) * count) // (2 * k) for j in range(k)]

    def step(self, scene: N.Scene, fused=None):
        """The next frame; `fused` overrides the constructor's for this step."""
        r = self.renderer
        fused = self.fused if fused is None else bool(fused)
        cfg = self.frame_config()
        r.upload(scene)
        subframes = scene.view()["subframes"]
        cam = N.Camera.of(subframes[len(subframes) // 2]["cam"])
        if self.adaptive_params is None and fused:
            _, acc, moments, albedo, normal_depth = r.render_with_features(cfg)
        else:
            if self.adaptive_params is not None:
                _, acc, moments, _ = r.render_adaptive(cfg, self.adaptive_params)
            else:
                _, acc, moments = r.render_moments(cfg, want_accum=True)
            albedo, normal_depth = r.render_features(cfg)
        if self.clamp_params is None and self.blur_cameras == 1:
            # in place: this frame's radiance and moments become the accumulated ones
            acc, moments, _ = r.temporal_accumulate(cam, acc, moments, albedo, normal_depth, self.history,
                                                    self.temporal_params, out_radiance=acc, out_moments=moments)
        else:
            from .denoise import TemporalClampParams
            p = self.clamp_params
            if p is None:
                p = TemporalClampParams.default(clamp_radius=0)
                if self.temporal_params is not None:
                    p.base = self.temporal_params
            cams = [subframes[k]["cam"] for k in self.blur_subframes(len(subframes))]
            # the moments in place; the radiance never with clamp_params: a clamp gathers it from neighbours
            acc, moments, _ = r.temporal_accumulate_clamped(cams, acc, moments, albedo, normal_depth, self.history, p,
                                                            out_radiance=acc if self.clamp_params is None else None,
                                                            out_moments=moments)
        out, bgra = r.denoise_guided(acc, albedo, normal_depth, moments, self.guided_params, want_bgra=True)
        self.history = (cam, acc, moments, albedo, normal_depth)
        self.frames += 1
        return bgra, out
