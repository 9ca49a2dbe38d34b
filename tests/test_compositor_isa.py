"""The compositor kernels as built (no GPU): the machine code of every volrender_ device function in librtxn.so, pinned by
tools/kernel_isa_hash.py's fingerprint (mangled name + code bytes).  The table was taken from the build BEFORE the plain and
the extended one-sample forward kernels were merged into one inlined body (fwd_body<MODE, COMPACT, AUX>), so it is what
guarantees that an instantiation through the body is the kernel it replaced; bench.py and profiles/ quote measurements of
these kernels only while their fingerprints hold.  Entries that the merge changed carry the new value and say so."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_isa_hash  # noqa: E402

LIB = os.path.join(ROOT, "rtx_nerf_amd", "librtxn.so")

WANT = {
    "_ZN12_GLOBAL__N_120volrender_aux_kernelILi0ELb0EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPfNS_7AuxArgsE":
        "0834b5edce4a6ee0",
    "_ZN12_GLOBAL__N_120volrender_aux_kernelILi0ELb1EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPfNS_7AuxArgsE":
        "ccaccd4679a43923",
    "_ZN12_GLOBAL__N_120volrender_aux_kernelILi1ELb0EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPfNS_7AuxArgsE":
        "d8b3536d04fa43de",
    # one-sample <RTXN_VR_NERF, COMPACT>: the address arithmetic of the loop is strength-reduced differently through the
    # inlined body (28 bytes longer; before the merge: 334345ed42fa0651)
    "_ZN12_GLOBAL__N_120volrender_aux_kernelILi1ELb1EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPfNS_7AuxArgsE":
        "df237d99705275ec",
    "_ZN12_GLOBAL__N_120volrender_fwd_kernelILi0ELb0EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPf":
        "8c71126c4d4decbd",
    "_ZN12_GLOBAL__N_120volrender_fwd_kernelILi0ELb1EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPf":
        "7870e68c16c29eeb",
    "_ZN12_GLOBAL__N_120volrender_fwd_kernelILi1ELb0EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPf":
        "d03747275d983799",
    # one-sample <RTXN_VR_NERF, COMPACT>: the address arithmetic of the loop is strength-reduced differently through the
    # inlined body (28 bytes longer; before the merge: 4438bfe73c7da554)
    "_ZN12_GLOBAL__N_120volrender_fwd_kernelILi1ELb1EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPf":
        "2ff581e67d5a4ea5",
    "_ZN12_GLOBAL__N_122volrender_l2_bg_kernelEPK15HIP_vector_typeIfLj4EEPKfPKiS7_iiS5_fPfP6__halfS8_PNS_5half4ENS_6BgArgsE":
        "3de71cc119afa1af",
    "_ZN12_GLOBAL__N_125volrender_aux_pair_kernelILi0ELb0EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPfNS_7AuxArgsE":
        "bd983d43795813b3",
    "_ZN12_GLOBAL__N_125volrender_aux_pair_kernelILi0ELb1EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPfNS_7AuxArgsE":
        "7c5f1e9025d83daf",
    "_ZN12_GLOBAL__N_125volrender_aux_pair_kernelILi1ELb0EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPfNS_7AuxArgsE":
        "685881b8976c48a5",
    "_ZN12_GLOBAL__N_125volrender_aux_pair_kernelILi1ELb1EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPfNS_7AuxArgsE":
        "17aeed69ae623c82",
    "_ZN12_GLOBAL__N_125volrender_bwd_nerf_kernelEPK6__halfPK15HIP_vector_typeIfLj4EEPKfPKiSA_iiPNS_5half4E":
        "b8d436696adebe54",
    "_ZN12_GLOBAL__N_125volrender_fwd_pair_kernelILi0ELb0EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPf":
        "cf97196abf306c0f",
    "_ZN12_GLOBAL__N_125volrender_fwd_pair_kernelILi0ELb1EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPf":
        "2c3c19374cb166d0",
    "_ZN12_GLOBAL__N_125volrender_fwd_pair_kernelILi1ELb0EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPf":
        "f353b8c5fa68e9b2",
    "_ZN12_GLOBAL__N_125volrender_fwd_pair_kernelILi1ELb1EEEvPK15HIP_vector_typeIfLj4EEPKiS6_PKfiiPf":
        "80021e9d17f9346b",
    "_ZN12_GLOBAL__N_125volrender_l2_fused_kernelEPK15HIP_vector_typeIfLj4EEPKfPKiS7_iiS5_fPfP6__halfS8_PNS_5half4E":
        "d1bc313372473022",
    "_ZN12_GLOBAL__N_127volrender_bwd_compat_kernelEPK6__halfPK15HIP_vector_typeIfLj4EEPKfPKiSA_iiPNS_5half4E":
        "2a13d105882c2ddc",
    "_ZN12_GLOBAL__N_128volrender_l2_bg_multi_kernelILi4EEEvPK15HIP_vector_typeIfLj4EEPKfPKiS8_iiS6_fPfP6__halfS9_PNS_5half4ENS_6BgArgsE":
        "c4c70c81e4b322ef",
    "_ZN12_GLOBAL__N_131volrender_l2_fused_multi_kernelILi4EEEvPK15HIP_vector_typeIfLj4EEPKfPKiS8_iiS6_fPfP6__halfS9_PNS_5half4E":
        "f581d528df1205b7",
}


def _volrender_functions():
    names = set()
    for co in kernel_isa_hash._code_objects(LIB):
        names.update(n for n in kernel_isa_hash._functions(co) if "volrender_" in n)
    return names


@pytest.fixture(scope="module")
def built():
    tools = [os.path.join(kernel_isa_hash.LLVM, t) for t in ("llvm-objcopy", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) or shutil.which(os.path.basename(t)) for t in tools):
        pytest.skip("librtxn.so or the LLVM binary tools are absent")


def test_the_compositor_device_functions_are_exactly_the_pinned_ones(built):
    """a body that was not inlined, or a new instantiation, shows up as a function that the table does not know"""
    assert _volrender_functions() == set(WANT)


@pytest.mark.parametrize("name", sorted(WANT))
def test_compositor_kernel_keeps_its_machine_code(built, name):
    assert kernel_isa_hash.kernel_isa_sha16([name]) == WANT[name]
