"""tools/isa_mix.py: instruction mix of one kernel / one loop of hipcc -S output (no GPU)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_mix.py")

ASM = """\
	.text
_Z5otherv:                              ; @_Z5otherv
	v_mov_b32_e32 v0, 0
	s_endpgm
.Lfunc_end0:
_Z6kernelv:                             ; @_Z6kernelv
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0
.LBB1_1:                                ; =>This Inner Loop Header: Depth=1
	ds_read_b128 v[4:7], v2
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_16x16x32_bf16 v[8:11], v[4:7], v[4:7], 0
	s_nop 5
	v_and_or_b32 v12, v8, s2, 1
	;;#ASMSTART
	v_min_f32 v13, v13, v12
	;;#ASMEND
	v_mov_b32_e32 v14, v13
	s_add_u32 s3, s3, 1
	s_cbranch_scc1 .LBB1_1
; %bb.2:
	global_store_dword v[0:1], v14, off
	s_endpgm
.Lfunc_end1:
"""


def run(tmp_path, *args):
    p = tmp_path / "k.s"
    p.write_text(ASM)
    return subprocess.run([sys.executable, TOOL, str(p), *args], capture_output=True, text=True, check=True).stdout


def test_loop_mix_counts_classes_and_nops_after_mfma(tmp_path):
    out = run(tmp_path, "_Z6kernelv", "--loop", "auto")
    assert "loop .LBB1_1" in out
    assert "instructions 9: matrix 1, other vector 3, scalar 2, LDS 1, vmem 0, smem 0, waits 1, s_nop 1" in out
    assert "s_nop wait states 6; s_nop right after a matrix instruction: 1 (6 wait states)" in out
    assert "v_min_f32" in out            # inline-asm lines count as instructions


def test_whole_kernel_and_line_range(tmp_path):
    out = run(tmp_path, "kernelv")   # unique substring of the symbol
    assert "whole kernel" in out and "global_store_dword" in out and "s_endpgm" in out
    out = run(tmp_path, "_Z6kernelv", "--lines", "10:12")
    assert "instructions 3: matrix 1, other vector 0, scalar 0, LDS 1, vmem 0, smem 0, waits 1, s_nop 0" in out


def test_ambiguous_symbol_is_an_error(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(ASM)
    r = subprocess.run([sys.executable, TOOL, str(p), "_Z"], capture_output=True, text=True)
    assert r.returncode != 0 and "matches 2 functions" in r.stderr
