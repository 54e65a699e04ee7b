"""tests/isa_util.py and tests/abi_util.py on a hand-written assembly text and stub objects: the shared checks read what the
text says and refuse what the copies they replaced refused.  Nothing is compiled; no GPU."""
import ctypes as C

import pytest

from abi_util import FAKE, filled, refused
from isa_util import assert_no_scratch, find, kernels, meta, scratch_bytes, vgprs

PLAIN, SPILL, INST = "_ZN3lrf7k_plainEPfi", "_ZN3lrf7k_spillEPfi", "_ZN3lrf6k_instILi8ELb1EEEvPf"


def _kernel(name, body, scratch, regs):
    return f"""\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
{body}\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_private_segment_fixed_size {scratch}
\t\t.amdhsa_next_free_vgpr {regs}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end_{name}:
; Kernel info:
; NumVgprs: {regs}
; ScratchSize: {scratch}
"""


ASM = (_kernel(PLAIN, "\tv_add_f32 v0, v1, v2\n", 0, 12)
       + _kernel(SPILL, "\tscratch_load_dword v0, off, off\n", 16, 40)
       + _kernel(INST, "\tv_mul_f32 v0, v1, v2\n", 0, 7))


def test_the_readers_return_what_the_text_says():
    assert list(kernels(ASM)) == [PLAIN, SPILL, INST]
    assert "v_add_f32" in kernels(ASM)[PLAIN] and "v_add_f32" not in kernels(ASM)[INST]
    assert [n for n, _ in find(ASM, r"k_(plain|inst)")] == [PLAIN, INST] and find(ASM, "k_instILi8E")[0][1] == kernels(ASM)[INST]
    with pytest.raises(AssertionError):
        find(ASM, "k_absent")
    assert meta(ASM, SPILL).startswith(".amdhsa_kernel " + SPILL) and ".amdhsa_next_free_vgpr 40" in meta(ASM, SPILL)
    assert ".end_amdhsa_kernel" not in meta(ASM, SPILL) and PLAIN not in meta(ASM, SPILL)
    assert [scratch_bytes(ASM, n) for n in (PLAIN, SPILL, INST)] == [0, 16, 0]
    assert [vgprs(ASM, n) for n in (PLAIN, SPILL, INST)] == [12, 40, 7]


def test_assert_no_scratch_passes_on_the_clean_kernels_in_each_mode():
    assert [n for n, _ in assert_no_scratch(ASM, ("k_plain",), match="exact")] == [PLAIN]
    assert [n for n, _ in assert_no_scratch(ASM, ("k_inst", "k_plain"), match="prefix")] == [INST, PLAIN]
    found = assert_no_scratch(ASM, ("k_inst", "k_plain"), match="search", total=2, body_too=True)
    assert found == [(INST, kernels(ASM)[INST]), (PLAIN, kernels(ASM)[PLAIN])]


@pytest.mark.parametrize("names,kw", [
    (("k_spill",), dict(match="exact")), (("k_spill",), dict(match="prefix")), (("k_spill",), dict(match="search", total=1)),   # scratch
    (("k_absent",), dict(match="exact")), (("k_absent",), dict(match="prefix")), (("k_absent",), dict(match="search", total=1)),  # no hit
    (("k_inst",), dict(match="exact")),                                  # a template instance is no hit for the plain name
    (("k_[a-z]+",), dict(match="exact")), (("k_",), dict(match="prefix")),                                                   # two hits
    (("k_plain", "k_inst"), dict(match="search", total=3)), (("k_",), dict(match="search", total=1)),                        # the total
])
def test_assert_no_scratch_refuses(names, kw):
    with pytest.raises(AssertionError):
        assert_no_scratch(ASM, names, **kw)


def test_body_too_refuses_a_scratch_instruction_the_metadata_does_not_show():
    asm = ASM.replace("v_mul_f32 v0, v1, v2", "scratch_load_dword v0, off, off")
    assert [n for n, _ in assert_no_scratch(asm, ("k_inst",), match="search", total=1)] == [INST]
    with pytest.raises(AssertionError):
        assert_no_scratch(asm, ("k_inst",), match="search", total=1, body_too=True)


def test_filled_sets_scalars_and_array_members():
    class S(C.Structure):
        _fields_ = [("p", C.c_void_p), ("n", C.c_int64), ("h", C.c_double), ("lo", C.c_double * 3), ("dims", C.c_int32 * 3)]
    a = filled(S, dict(p=FAKE, n=9, h=0.5, lo=(0.0,) * 3, dims=(4, 4, 4)))
    assert (a.p, a.n, a.h, list(a.lo), list(a.dims)) == (FAKE, 9, 0.5, [0.0, 0.0, 0.0], [4, 4, 4])
    b = filled(S, dict(p=FAKE, n=9, dims=(4, 4, 4)), p=None, n=-1, dims=[7, 8], lo=(1.0, 2.0, 3.0))
    assert (b.p, b.n, b.h, list(b.lo), list(b.dims)) == (None, -1, 0.0, [1.0, 2.0, 3.0], [7, 8, 4])
    with pytest.raises(AttributeError):
        filled(S, {}, absent=(1, 2))


def test_refused_needs_a_refusal_and_the_symbol_in_front():
    class Lib:
        def lrf_last_error(self):
            return b"lrf_thing: null argument"
    assert refused(Lib(), 1) == refused(Lib(), -3, "lrf_thing") == "lrf_thing: null argument"
    with pytest.raises(AssertionError):
        refused(Lib(), 0)
    with pytest.raises(AssertionError):
        refused(Lib(), 1, "lrf_other")
    with pytest.raises(AssertionError):
        refused(Lib(), 1, "lrf_thin")                                   # the whole name, then ": "
