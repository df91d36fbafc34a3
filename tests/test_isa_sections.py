"""tools/isa_sections.py on a short synthetic listing: the counts by mnemonic
prefix, the labelled ranges, the table file and the command line."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_sections as T  # noqa: E402

LISTING = """\
\t.text
\t.globl\t_Z5otherv
_Z5otherv:
\tv_mov_b32_e32 v0, 0
\ts_endpgm
.Lfunc_end0:
\t.globl\t_Z4walkv
\t.type\t_Z4walkv,@function
_Z4walkv:                               ; @_Z4walkv
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\tv_mov_b32_e32 v1, 0                     ; a comment with s_mov_b32 in it
.LBB1_1:                                ; =>This Inner Loop Header: Depth=1
\tglobal_load_dwordx4 v[2:5], v1, s[0:1]
\tds_read2st64_b32 v[6:7], v1 offset1:1
\tv_add_f32_e32 v2, v2, v6
\tv_max3_f32 v2, v2, v3, v4
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB1_3
; %bb.2:
\tbuffer_load_dword v8, v1, s[8:11], 0 offen
\tscratch_load_dword v9, off, off
\tflat_load_dword v10, v[2:3]
\tds_write2st64_b32 v1, v6, v7 offset1:1
.LBB1_3:
\ts_or_b64 exec, exec, s[2:3]
\ts_nop 0
\ts_cbranch_scc1 .LBB1_1
; %bb.4:
\ts_endpgm
.Lfunc_end1:
\t.size\t_Z4walkv, .Lfunc_end1-_Z4walkv
\t.set _Z4walkv.num_vgpr, 11
"""


def test_classes_go_by_prefix():
    assert T.classify("s_mov_b32") == "scalar" and T.classify("s_waitcnt") == "scalar"
    assert T.classify("s_cbranch_execz") == "branch" and T.classify("s_branch") == "branch" and T.classify("s_endpgm") == "branch"
    assert T.classify("v_pk_mov_b32") == "valu" and T.classify("v_cmp_class_f32_e64") == "valu"
    for m in ("global_load_dwordx4", "buffer_load_dword", "flat_store_dword", "scratch_load_dword"):
        assert T.classify(m) == "vmem"
    assert T.classify("ds_read_b64") == "lds"
    assert T.classify("image_sample") == "other"


def test_whole_kernel_counts():
    rows = T.sections(LISTING, "_Z4walkv")
    assert [n for n, _ in rows] == ["kernel"]
    c = rows[0][1]
    assert c == {"scalar": 5, "valu": 3, "vmem": 4, "lds": 2, "branch": 3, "other": 0, "total": 17}
    # the neighbouring function is not counted, and neither are comments, labels and directives
    assert T.sections(LISTING, "_Z5otherv")[0][1]["total"] == 2


def test_labelled_ranges():
    ranges = [["head", "", ".LBB1_1"], ["loop", ".LBB1_1", ".LBB1_3"], ["tail", ".LBB1_3", ""]]
    rows = dict(T.sections(LISTING, "_Z4walkv", ranges))
    assert rows["head"] == {"scalar": 2, "valu": 1, "vmem": 0, "lds": 0, "branch": 0, "other": 0, "total": 3}
    assert rows["loop"] == {"scalar": 1, "valu": 2, "vmem": 4, "lds": 2, "branch": 1, "other": 0, "total": 10}
    assert rows["tail"] == {"scalar": 2, "valu": 0, "vmem": 0, "lds": 0, "branch": 2, "other": 0, "total": 4}
    assert sum(rows[k]["total"] for k in ("head", "loop", "tail")) == rows["kernel"]["total"]


def test_unknown_names_are_errors():
    with pytest.raises(KeyError):
        T.sections(LISTING, "_Z7missingv")
    with pytest.raises(KeyError):
        T.sections(LISTING, "_Z4walkv", [["x", ".LBB9_9", ""]])
    with pytest.raises(ValueError):
        T.sections(LISTING, "_Z4walkv", [["x", ".LBB1_3", ".LBB1_1"]])


def test_command_line_with_a_table(tmp_path):
    lst, tab = tmp_path / "unit.s", tmp_path / "ranges.json"
    lst.write_text(LISTING)
    tab.write_text(json.dumps({"walk": [["loop", ".LBB1_1", ".LBB1_3"]]}))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_sections.py"), str(lst), "_Z4walkv",
                          "--ranges", str(tab), "--key", "walk"], capture_output=True, text=True, check=True).stdout
    lines = out.strip().split("\n")
    assert lines[0].split() == ["range", "total", "scalar", "valu", "vmem", "lds", "branch", "other"]
    assert lines[1].split() == ["kernel", "17", "5", "3", "4", "2", "3", "0"]
    assert lines[2].split() == ["loop", "10", "1", "2", "4", "2", "1", "0"]
