"""tools/isa_diff.py, the device-code comparison a refactor of the kernel units
has to pass: its normaliser ignores what differs between two builds of the same
code (comments, the function number in local labels) and nothing else, and a
unit compared with itself is reported identical. CPU only (device-only
compiles, no GPU)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)

A = """\
_Z1kv:                                  ; @_Z1kv
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0    ; a comment
\ts_cbranch_scc1 .LBB3_2
.LBB3_2:                                ; %exit
\ts_endpgm
.Lfunc_end3:
"""
B = """\
_Z1kv:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0    ; another comment

\ts_cbranch_scc1 .LBB0_2
.LBB0_2:
\ts_endpgm
.Lfunc_end0:
"""


def test_normaliser_ignores_comments_and_function_numbers():
    assert isa_diff.normalise(A, "_Z1kv") == isa_diff.normalise(B, "_Z1kv")


def test_normaliser_keeps_instructions():
    assert isa_diff.normalise(A, "_Z1kv") != isa_diff.normalise(B.replace("0x0", "0x8"), "_Z1kv")
    assert isa_diff.normalise(A, "_Z1kv") != isa_diff.normalise(B.replace(".LBB0_2\n", ".LBB0_3\n"), "_Z1kv")


def test_kernel_name_drops_parameters():
    assert isa_diff.kernel_name("void mraft::(anonymous namespace)::k<1, 0>(mraft::T, int (*)(int))") == \
        "mraft::(anonymous namespace)::k<1, 0>"
    assert isa_diff.kernel_name("mraft::(anonymous namespace)::k_p1(mraft::Dev, int const*)") == \
        "mraft::(anonymous namespace)::k_p1"


@pytest.mark.skipif(not os.path.exists(isa_diff.HIPCC), reason="no hipcc")
def test_unit_identical_to_itself(tmp_path):
    old = isa_diff.tree_kernels(ROOT, str(tmp_path), "old", ["mraft_elect.hip"])
    new = isa_diff.tree_kernels(ROOT, str(tmp_path), "new", ["mraft_elect.hip"])
    rows = isa_diff.compare(old, new)
    # k_election_rounds<1..8>, without and with the reachability pack
    assert len(rows) == 16 and all(v == "IDENTICAL" for v, _ in rows), rows
    # and a kernel whose code changed is told apart
    name = next(iter(new))
    new[name] = (new[name][0], new[name][1][:-1])
    assert [v for v, what in isa_diff.compare(old, new) if name in what] == ["DIFFERS"]
    del new[name]
    assert [v for v, what in isa_diff.compare(old, new) if name in what] == ["ONLY-IN-ONE"]
