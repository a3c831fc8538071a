"""tools/kernel_streams.py's two normalisations, on literal instruction lines and names (no library, no disassembler):
the pc-relative mask takes the literals of the pair behind `s_getpc_b64` on that instruction's registers and nothing
else, and the name rule drops the fused four-step kernel's retired `, 2, 0` and nothing else."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_streams as ks          # noqa: E402

FUSED = ("void rpf::(anonymous namespace)::fourstep_fused_kernel<rpf::(anonymous namespace)::Split<512, 512>, false, true%s>"
         "(unsigned char const*, int, HIP_vector_type<float, 2u> const*)")


def test_pair_behind_getpc_is_masked():
    a = ["s_load_dwordx2 s[2:3], s[0:1], 0x0", "s_getpc_b64 s[4:5]", "s_add_u32 s4, s4, 0xfffa3458",
         "s_addc_u32 s5, s5, -1", "s_add_u32 s6, s6, 0xfffa3458"]
    b = [a[0], a[1], "s_add_u32 s4, s4, 0xfffa33d8", "s_addc_u32 s5, s5, -1", a[4]]
    ma, mb = ks.mask_pc_relative(a), ks.mask_pc_relative(b)
    assert ma == mb and ks.digest(a) != ks.digest(b)
    assert ma == [a[0], a[1], "s_add_u32 s4, s4, " + ks.PCREL, "s_addc_u32 s5, s5, " + ks.PCREL, a[4]]
    assert a[2] == "s_add_u32 s4, s4, 0xfffa3458"          # the input is left alone


def test_same_add_without_getpc_is_not_masked():
    for lines in (["s_mov_b64 s[4:5], s[2:3]", "s_add_u32 s4, s4, 0xfffa3458", "s_addc_u32 s5, s5, -1"],
                  ["s_getpc_b64 s[8:9]", "s_add_u32 s4, s4, 0xfffa3458", "s_addc_u32 s5, s5, -1"],          # other registers
                  ["s_getpc_b64 s[4:5]", "s_nop 0", "s_add_u32 s4, s4, 0xfffa3458", "s_addc_u32 s5, s5, -1"],   # not directly behind
                  ["s_getpc_b64 s[4:5]", "s_add_u32 s4, s4, 0xfffa3458"]):                                   # half a pair
        assert ks.mask_pc_relative(lines) == lines


def test_add_with_another_destination_is_not_masked():
    lines = ["s_getpc_b64 s[4:5]", "s_add_u32 s6, s4, 0xfffa3458", "s_addc_u32 s7, s5, -1"]
    assert ks.mask_pc_relative(lines) == lines
    other = [lines[0], "s_add_u32 s6, s4, 0xfffa33d8", lines[2]]
    assert ks.digest(ks.mask_pc_relative(lines)) != ks.digest(ks.mask_pc_relative(other))


def test_name_normalisation():
    assert ks.drop_fused_defaults(FUSED % ", 2, 0") == FUSED % ""
    assert ks.drop_fused_defaults(FUSED % "") == FUSED % ""
    for kept in (FUSED % ", 1, 0", FUSED % ", 2, 1", FUSED % ", 3, 0"):
        assert ks.drop_fused_defaults(kept) == kept
    k1 = "void rpf::fft_accum_kernel<rpf::Geom<4096, 16>, 256, 2, false, true, 2, 0>(unsigned char const*, long)"
    assert ks.drop_fused_defaults(k1) == k1
