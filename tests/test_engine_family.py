"""The rule that picks an engine's kernel family, csrc/engine_family.h's select_family (through
tests/emul/engine_family_emul.cpp, compiled here), against the chain of seven interdependent bools rpf_engine_create
held before the rule became one priority list: the same seven names and expressions, and the order in which the
engine's ladders let them win.  The two forms are written differently on purpose; what is checked is that they agree on
every query that can occur -- the choice and the refusals."""
import ctypes
import itertools
import os
import subprocess

import pytest

from helpers import ROOT

FAMILIES = ["K1", "Mixed", "FourStep", "Bluestein", "BigBluestein", "Generic", None]      # enum class Family; None: no kernel
# FamilyQuery's bools in declaration order: the bit positions of the shim
BOOLS = ["cu8", "stats", "windowed", "flag_catch_all", "flag_no_mixed_radix", "flag_fourstep_fused",
         "k1_v0", "k1", "mixed", "fourstep", "bluestein", "bigblu", "generic"]


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("engine_family") / "librpf_emul_engine_family.so")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", lib,
                    os.path.join(ROOT, "tests", "emul", "engine_family_emul.cpp")], check=True)
    lib = ctypes.CDLL(lib)
    lib.rpf_emul_select_family.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    lib.rpf_emul_select_family.restype = ctypes.c_int

    def call(N, variant, **q):
        bits = sum(1 << k for k, name in enumerate(BOOLS) if q[name])
        return FAMILIES[lib.rpf_emul_select_family(N, variant, bits)]
    return call


def parent_chain(N, variant, cu8, stats, windowed, flag_catch_all, flag_no_mixed_radix, flag_fourstep_fused,
                 k1_v0, k1, mixed, fourstep, bluestein, bigblu, generic):
    """rpf_engine_create's chain, literally: `x_supported` is what the build has at N, the seven bools are the chain's.
    Returns the family the engine's ladders then ran (generic, else mixed, bluestein, bigblu, fourstep, else K1), or
    None where create said "No gfx950 kernel"."""
    native_k1 = k1_v0
    kernel_supported, mixed_supported, fourstep_supported = k1, mixed, fourstep
    bluestein_supported, bigblu_supported, generic_supported = bluestein, bigblu, generic
    catch_all = flag_catch_all or ((not cu8 or stats) and not native_k1)
    windowed_32768 = N == 32768 and windowed and variant == 0
    mixed = (not catch_all and mixed_supported and not windowed_32768
             and not (flag_no_mixed_radix or flag_fourstep_fused))
    fourstep = not catch_all and not mixed and fourstep_supported and variant == 0
    bluestein = not catch_all and not mixed and bluestein_supported and variant == 0
    bigblu = not catch_all and not mixed and bigblu_supported and variant == 0
    tuned = not catch_all and (fourstep or mixed or bluestein or bigblu
                               or (kernel_supported and (cu8 or variant == 0)))
    generic = not tuned and variant == 0 and generic_supported
    if not tuned and not generic:
        return None
    if generic:
        return "Generic"
    if mixed:
        return "Mixed"
    if bluestein:
        return "Bluestein"
    if bigblu:
        return "BigBluestein"
    if fourstep:
        return "FourStep"
    return "K1"


def queries():
    """Every FamilyQuery that can occur: at most one of four-step, Bluestein and large Bluestein at an N, and K1 at the
    asked variant is K1 at variant 0 when that is what was asked."""
    for N, variant in itertools.product((32768, 4096), (0, 1)):
        for values in itertools.product((False, True), repeat=len(BOOLS)):
            q = dict(zip(BOOLS, values))
            if q["fourstep"] + q["bluestein"] + q["bigblu"] > 1:
                continue
            if variant == 0 and q["k1"] != q["k1_v0"]:
                continue
            yield N, variant, q


def test_select_family_agrees_with_the_chain_it_replaced(select):
    seen, refused, checked = set(), 0, 0
    for N, variant, q in queries():
        want = parent_chain(N, variant, **q)
        got = select(N, variant, **q)
        assert got == want, (N, variant, q)        # (the refusals are exactly the chain's: None == None)
        seen.add(want)
        refused += want is None
        checked += 1
    assert checked == 2 * (4096 + 2048)     # per N: 2^13 / 2 (one of the three or none) at variant 1, half of that at 0
    assert seen == {None, "K1", "Mixed", "FourStep", "Bluestein", "BigBluestein", "Generic"}
    assert 0 < refused < checked


def test_the_rules_the_comments_state(select):
    base = dict.fromkeys(BOOLS, False)
    base.update(cu8=True, generic=True)
    # 32768 is served twice: plain runs on the split form, windowed runs on the four-step kernels
    both = dict(base, mixed=True, fourstep=True)
    assert select(32768, 0, **both) == "Mixed"
    assert select(32768, 0, **dict(both, windowed=True)) == "FourStep"
    assert select(4096, 0, **dict(both, windowed=True)) == "Mixed"
    # asking for the fused kernel, or for no mixed radix, is asking for what is behind the mixed kernels
    assert select(32768, 0, **dict(both, flag_fourstep_fused=True)) == "FourStep"
    assert select(32768, 0, **dict(both, flag_no_mixed_radix=True)) == "FourStep"
    # signed formats and statistics: K1 where K1 has the size, else the catch-all path whatever else serves the size
    k1 = dict(base, k1_v0=True, k1=True)
    assert select(4096, 0, **dict(k1, cu8=False)) == "K1" and select(4096, 0, **dict(k1, stats=True)) == "K1"
    assert select(4096, 0, **dict(both, cu8=False)) == "Generic" and select(4096, 0, **dict(both, stats=True)) == "Generic"
    assert select(4096, 0, **dict(k1, flag_catch_all=True)) == "Generic"
    assert select(4096, 0, **dict(k1, flag_catch_all=True, generic=False)) is None
