"""CPU checks of the assembly normaliser of tools/kernel_isa.py (no hipcc)."""

import importlib.util
import os

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "tools", "kernel_isa.py")
_spec = importlib.util.spec_from_file_location("kernel_isa", _PATH)
K = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K)


def _func(n, sym, body):
    return f"""\t.protected\t{sym}
\t.globl\t{sym}
\t.p2align\t8
\t.type\t{sym},@function
{sym}:                                  ; @{sym}
; %bb.0:
{body}
.Lfunc_end{n}:
\t.size\t{sym}, .Lfunc_end{n}-{sym}
\t.section\t.AMDGPU.csdata,"",@progbits
; NumVgprs: {7 + n}
"""


def _body(n, add="v_add_f32_e32 v0, v0, v1", note="first"):
    return f"""\ts_load_dwordx2 s[0:1], s[4:5], 0x0  ; {note} comment
\ts_waitcnt lgkmcnt(0)
\t.loc\t1 {n} 3
.LBB{n}_1:                                ; =>This Inner Loop Header: Depth=1
\t{add}
\ts_cbranch_scc1 .LBB{n}_1
; %bb.2:
\ts_endpgm"""


A = _func(0, "_Z3foov", _body(0)) + _func(1, "_Z3barv", _body(1, "v_mul_f32_e32 v0, v0, v1"))
# same code: functions swapped and renumbered, other comments and directives
B = (_func(0, "_Z3barv", _body(0, "v_mul_f32_e32 v0, v0, v1", note="other"))
     + "\t.text\n"
     + _func(3, "_Z3foov", _body(3, note="another")))
# one instruction of foo changed
C = _func(0, "_Z3foov", _body(0, "v_sub_f32_e32 v0, v0, v1")) + _func(1, "_Z3barv", _body(1, "v_mul_f32_e32 v0, v0, v1"))


def test_normaliser_keeps_the_instructions():
    k = K.kernels(A)
    assert set(k) == {"_Z3foov", "_Z3barv"}
    assert k["_Z3foov"].splitlines() == [
        "s_load_dwordx2 s[0:1], s[4:5], 0x0",
        "s_waitcnt lgkmcnt(0)",
        ".LBB_1:",
        "v_add_f32_e32 v0, v0, v1",
        "s_cbranch_scc1 .LBB_1",
        "s_endpgm",
    ]


def test_labels_comments_and_order_compare_same():
    assert K.compare(K.kernels(A), K.kernels(B)) == {"_Z3barv": "same", "_Z3foov": "same"}


def test_changed_instruction_compares_diff():
    assert K.compare(K.kernels(A), K.kernels(C)) == {"_Z3barv": "same", "_Z3foov": "DIFF"}


def test_added_and_removed():
    only_foo = _func(0, "_Z3foov", _body(0))
    assert K.compare(K.kernels(A), K.kernels(only_foo)) == {"_Z3barv": "removed", "_Z3foov": "same"}
    assert K.compare(K.kernels(only_foo), K.kernels(A)) == {"_Z3barv": "added", "_Z3foov": "same"}


def test_resource_remarks():
    rem = """\
a.hip:9:1: remark: Function Name: _Z3foov [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     TotalSGPRs: 22 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     VGPRs: 230 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     AGPRs: 160 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     ScratchSize [bytes/lane]: 316 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     Occupancy [waves/SIMD]: 1 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     SGPRs Spill: 16 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     VGPRs Spill: 98 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
"""
    assert K.resources(rem) == {"_Z3foov": {
        "vgpr": "230", "agpr": "160", "scratch": "316", "occ": "1",
        "sspill": "16", "vspill": "98", "lds": "0"}}


def test_rename_pairs_by_demangled_name():
    names = {"_Z3foov": "foo<1>", "_Z3barv": "bar", "_Z3quxv": "qux<1, false>",
             "_Z3zapv": "zap<1, false>"}
    ren = [K.rename_arg(r"foo<(.*)>=qux<\1, false>")]
    base = K.kernels(A)

    def run(new_foo_sym, add):
        new = K.kernels(_func(0, new_foo_sym, _body(0, add))
                        + _func(1, "_Z3barv", _body(1, "v_mul_f32_e32 v0, v0, v1")))
        to = K.renamed(base, new, names, ren)
        return to, K.compare({to.get(s, s): t for s, t in base.items()}, new)

    # foo<1> -> qux<1, false>, equal text / one instruction changed
    to, res = run("_Z3quxv", "v_add_f32_e32 v0, v0, v1")
    assert to == {"_Z3foov": "_Z3quxv"}
    assert res == {"_Z3barv": "same", "_Z3quxv": "same"}
    _, res = run("_Z3quxv", "v_sub_f32_e32 v0, v0, v1")
    assert res == {"_Z3barv": "same", "_Z3quxv": "DIFF"}
    # no kernel carries the renamed name: nothing is paired
    to, res = run("_Z3zapv", "v_add_f32_e32 v0, v0, v1")
    assert to == {}
    assert res == {"_Z3barv": "same", "_Z3foov": "removed", "_Z3zapv": "added"}
