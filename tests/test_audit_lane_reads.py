"""tools/audit_asm_hazards.py, the wait states around an inline-asm lane read (the gfx940 family's VALUWriteVGPRReadlaneRead = 1
and VALUWriteSGPRVALURead = 2, which hipcc does not insert around inline asm): bad and good snippets."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "_ZN3pgd6kernelEv:\n\tv_mfma_f32_16x16x32_bf16 v[100:103], v[104:107], v[108:111], v[100:103]\n"
TAIL = "\ts_endpgm\n"
ASM = "\t;;#ASMSTART\n%s\t;;#ASMEND\n"

CASES = {
    # the multiply's result read by the asm in the next slot
    "bad_vgpr_then_readfirstlane": ("\tv_mul_f32_e32 v2, s14, v2\n" + ASM % "\tv_readfirstlane_b32 s4, v2\n\ts_nop 1\n", False),
    "bad_vgpr_then_readlane": ("\tv_add_f32_e32 v9, v1, v2\n" + ASM % "\tv_readlane_b32 s4, v9, 3\n\ts_nop 1\n", False),
    # the SGPR the asm wrote read as an operand one wait state on
    "bad_sgpr_read_at_once": ("\tv_mul_f32_e32 v2, s14, v2\n\ts_nop 0\n" + ASM % "\tv_readfirstlane_b32 s4, v2\n" + "\tv_fma_f32 v7, s4, v6, v5\n", False),
    "bad_sgpr_read_one_state_on": ("\tv_mov_b32_e32 v3, 0\n" + ASM % "\tv_readfirstlane_b32 s4, v2\n\ts_nop 0\n" + "\tv_mul_f32_e32 v7, s4, v6\n", False),
    "good_padded": ("\tv_mul_f32_e32 v2, s14, v2\n" + ASM % "\ts_nop 0\n\tv_readfirstlane_b32 s4, v2\n\ts_nop 1\n" + "\tv_fma_f32 v7, s4, v6, v5\n", True),
    "good_other_register": ("\tv_mul_f32_e32 v3, s14, v2\n" + ASM % "\tv_readfirstlane_b32 s4, v2\n\ts_nop 1\n", True),
    "good_two_instructions_between": ("\tv_mul_f32_e32 v2, s14, v2\n\tv_cmp_lt_u32_e32 vcc, 47, v0\n" + ASM % "\tv_readfirstlane_b32 s4, v2\n"
                                      + "\ts_mov_b64 s[6:7], 0\n\ts_mov_b64 s[8:9], 0\n\tv_fma_f32 v7, s4, v6, v5\n", True),
    # hipcc's own lane reads are its own business: it pads them itself
    "good_compiler_readlane": ("\tv_mul_f32_e32 v2, s14, v2\n\tv_readfirstlane_b32 s4, v2\n", True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_lane_read_wait_states(tmp_path, name):
    body, ok = CASES[name]
    f = tmp_path / "k.s"
    f.write_text(HEAD + body + TAIL)
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "audit_asm_hazards.py"), str(f)], capture_output=True, text=True)
    assert (run.returncode == 0) == ok, run.stdout
    assert ("lane read without its wait states" in run.stdout) == (not ok), run.stdout
