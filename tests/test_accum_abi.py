"""The progressive accumulator (ptg_accum_*) exists at every layer that needs
no GPU: the header declares the four entries, both libraries export them,
native.py binds them and mirrors the 64-byte ptg_accum, and the checkpoint
file's pack / unpack keep every bit and refuse what is no checkpoint."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, N

ENTRIES = ("ptg_accum_state_bytes", "ptg_accum_begin", "ptg_accum_add", "ptg_accum_resolve")
HEADER = os.path.join(ROOT, "include", "ptg.h")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def test_the_header_declares_the_entries_and_the_abi_version_stays(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in ENTRIES:
        assert re.search(r"\b%s\s*\(" % f, text), f
    assert native_lib.ptg_abi_version() == 1
    assert re.search(r"#define\s+PTG_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+PTG_ACCUM_MOMENTS\s+1u", text) and re.search(r"#define\s+PTG_ACCUM_FEATURES\s+2u", text)
    # the size is pinned where the compiler sees it
    assert re.search(r"static_assert\(sizeof\(ptg_accum\) == 64", text)


def test_both_libraries_export_them():
    certfail = os.path.join(os.path.dirname(N.LIB_PATH), "libptg_certfail.so")
    for path in (N.LIB_PATH, certfail):
        missing = [f for f in ENTRIES if f not in _exports(path)]
        assert not missing, (path, missing)


def test_native_binds_them(native_lib):
    U32, P, I = C.c_uint32, C.c_void_p, C.c_int
    assert native_lib.ptg_accum_state_bytes.restype is C.c_size_t
    assert list(native_lib.ptg_accum_state_bytes.argtypes) == [U32] * 3
    assert list(native_lib.ptg_accum_begin.argtypes) == [P, P] + [U32] * 6 + [P, P]
    assert list(native_lib.ptg_accum_add.argtypes) == [P, P, P, U32]
    assert list(native_lib.ptg_accum_resolve.argtypes) == [P, P, P, I] + [P] * 5
    for f in ENTRIES[1:]:
        assert getattr(native_lib, f).restype is I


def test_the_ctypes_mirror_is_the_64_byte_header():
    assert C.sizeof(N.Accum) == 64
    offsets = {name: getattr(N.Accum, name).offset for name, _ in N.Accum._fields_}
    assert offsets == {"magic": 0, "version": 4, "cfg": 8, "x0": 32, "y0": 36, "w": 40, "h": 44, "flags": 48,
                       "sample_begin": 52, "sample_next": 56, "reserved": 60}
    assert N.ACCUM_MAGIC == int.from_bytes(b"PTGA", "little") == 0x41475450 and N.ACCUM_VERSION == 1


def test_state_bytes_for_the_four_flag_combinations(native_lib):
    w, h = 29, 19
    for flags, planes in ((0, 1), (N.ACCUM_MOMENTS, 2), (N.ACCUM_FEATURES, 3), (N.ACCUM_MOMENTS | N.ACCUM_FEATURES, 4)):
        assert N.accum_plane_count(flags) == planes
        assert native_lib.ptg_accum_state_bytes(w, h, flags) == planes * w * h * 16
    # no 32-bit overflow: 65536 x 65536 pixels of four planes
    assert native_lib.ptg_accum_state_bytes(1 << 16, 1 << 16, 3) == 4 * (1 << 32) * 16
    assert native_lib.ptg_accum_state_bytes(w, h, 4) == 0          # unknown flag bits


def test_the_entries_reject_a_null_context(native_lib):
    hdr = N.Accum()
    assert native_lib.ptg_accum_begin(None, None, 0, 0, 1, 1, 0, 0, C.byref(hdr), None) == -1
    assert native_lib.ptg_accum_add(None, C.byref(hdr), None, 1) == -1
    assert native_lib.ptg_accum_resolve(None, C.byref(hdr), None, 0, None, None, None, None, None) == -1


def _header(flags=3, w=5, h=3, begin=2, nxt=7):
    return N.Accum(N.ACCUM_MAGIC, N.ACCUM_VERSION, N.RenderConfig.make(16, 9, 24, 7), 4, 2, w, h, flags, begin, nxt, 0)


def _planes(flags=3, w=5, h=3):
    rng = np.random.default_rng(11)
    p = rng.integers(0, 1 << 32, (N.accum_plane_count(flags), h, w, 4), dtype=np.uint64).astype(np.uint32)
    p[0, 0, 0] = (0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000)   # quiet NaNs with payloads, a signalling NaN, -0
    if flags & N.ACCUM_MOMENTS:
        p[1, :, :, 2] = np.arange(h * w, dtype=np.uint32).reshape(h, w) + 3   # n: small integers, denormals as floats
    return p


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_pack_and_unpack_keep_every_bit(flags, tmp_path):
    hdr, planes = _header(flags), _planes(flags)
    # the state as the accumulator hands it over: float32, and as raw bytes
    for state in (planes.view(np.float32), planes.view(np.uint8).reshape(-1)):
        words, packed = N.accum_pack(hdr, state)
        assert words.dtype == np.uint32 and words.shape == (16,)
        assert packed.dtype == np.uint32 and packed.shape == planes.shape and np.array_equal(packed, planes)
        back, unpacked = N.accum_unpack(words, packed)
        assert bytes(back) == bytes(hdr) and np.array_equal(unpacked, planes)
    path = str(tmp_path / "checkpoint.npz")
    N.accum_save(path, hdr, planes.view(np.float32))
    assert os.path.exists(path)
    back, unpacked = N.accum_load(path)
    assert bytes(back) == bytes(hdr)
    assert unpacked.dtype == np.uint32 and np.array_equal(unpacked, planes)
    assert back.sample_begin == 2 and back.sample_next == 7 and back.cfg.max_bounces == 7
    if flags & N.ACCUM_MOMENTS:
        assert unpacked[1, 2, 4, 2] == 17


def test_unpack_refuses_what_is_no_checkpoint(tmp_path):
    hdr, planes = _header(), _planes()
    words, packed = N.accum_pack(hdr, planes)
    bad = words.copy()
    bad[0] ^= 1
    with pytest.raises(ValueError, match="magic"):
        N.accum_unpack(bad, packed)
    bad = words.copy()
    bad[1] = 2
    with pytest.raises(ValueError, match="version"):
        N.accum_unpack(bad, packed)
    with pytest.raises(ValueError, match="planes"):      # three planes under flags that say four
        N.accum_unpack(words, packed[:3])
    with pytest.raises(ValueError, match="planes"):      # the header of a state without features, four planes
        N.accum_unpack(N.accum_pack(_header(flags=1), _planes(flags=1))[0], packed)
    with pytest.raises(ValueError, match="planes"):      # another rectangle
        N.accum_unpack(words, packed[:, :, :4])
    with pytest.raises(ValueError, match="planes"):      # floats are not the file's format
        N.accum_unpack(words, packed.view(np.float32))
    bad = words.copy()
    bad[12] = 7
    with pytest.raises(ValueError, match="flags"):
        N.accum_unpack(bad, packed)
    with pytest.raises(ValueError, match="16"):
        N.accum_unpack(words[:15], packed)
    with pytest.raises(ValueError):                      # a state of another size than the header's
        N.accum_pack(hdr, planes[:3])
    path = str(tmp_path / "other.npz")
    np.savez(path, something=np.zeros(3))
    with pytest.raises(ValueError, match="no accumulator checkpoint"):
        N.accum_load(path)


def test_the_renderer_has_the_accumulator_and_the_generator():
    from ptlumi.renderer import Accumulator, GpuRenderer
    p = inspect.signature(Accumulator.__init__).parameters
    assert list(p)[:7] == ["self", "renderer", "cfg", "rect", "moments", "features", "sample_begin"]
    assert p["rect"].default is None and p["moments"].default is True and p["features"].default is True
    assert p["sample_begin"].default == 0
    for name in ("add", "resolve", "save", "load", "samples_done"):
        assert hasattr(Accumulator, name), name
    assert inspect.signature(Accumulator.resolve).parameters["by_samples"].default is False
    assert inspect.isgeneratorfunction(GpuRenderer.render_progressive)
    assert list(inspect.signature(GpuRenderer.render_progressive).parameters)[:4] == ["self", "cfg", "steps", "rect"]
