"""ptg_render_with_features exists at every layer: the libraries export it,
native.py binds its 13 arguments, the header declares it and the renderer
has the method that calls it (no GPU needed)."""
import ctypes as C
import inspect
import os
import subprocess

from conftest import N


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def test_the_libraries_export_the_entry():
    assert "ptg_render_with_features" in _exports(N.LIB_PATH)
    certfail = os.path.join(os.path.dirname(N.LIB_PATH), "libptg_certfail.so")
    assert "ptg_render_with_features" in _exports(certfail)


def test_the_header_declares_it_and_the_abi_version_stays():
    assert "ptg_render_with_features" in N.exported_symbols()
    assert N.lib().ptg_abi_version() == 1


def test_native_binds_13_arguments():
    fn = N.lib().ptg_render_with_features
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 13
    # context, config, the rectangle and the sample range, then five device pointers
    assert list(fn.argtypes[2:8]) == [C.c_uint32] * 6
    assert list(fn.argtypes[:2]) + list(fn.argtypes[8:]) == [C.c_void_p] * 7


def test_the_renderer_has_the_method_and_the_routes_their_switch():
    from ptlumi.renderer import GpuRenderer, TemporalDenoiser
    p = inspect.signature(GpuRenderer.render_with_features).parameters
    assert list(p) == ["self", "cfg", "rect", "samples", "want_moments"]
    assert p["want_moments"].default is True
    for route in (GpuRenderer.render_denoised, GpuRenderer.render_denoised_guided, TemporalDenoiser.step):
        assert "fused" in inspect.signature(route).parameters, route.__name__
    assert inspect.signature(GpuRenderer.render_denoised).parameters["fused"].default is True
