"""The Gram kernel's k-loop with the stage as a compile-time constant (gram_streamk_glds_body, GV & 512), read from the
generated code (CPU only: hipcc cross-compiles without a GPU), in the style of tests/test_isa_cpu.py.

The loop runs as trips of three k-steps on stages 0, 1, 2 and a tail of one to four steps.  What the change is about is
which instructions stand between the MFMAs, and a source change that looks innocent can bring the old ones back (a
fragment address rebuilt per step, a stage base selected at run time, a 64-bit compare on the vector ALU) or make the
register allocator move accumulators between the register files -- results stay right and the parity tests stay green.
So the main loop of the production instantiation (224 | 512 = 736) and of the batch kernel must hold three k-steps,
none of the instructions the change removed, and fewer instructions that are not MFMAs per k-step than the loop rolled
over a runtime stage index (224), which is compiled in the same run and counted the same way."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc", "dopt_kernels.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

NEW = ["gram_streamk_glds_kernelINS_4TileILi256ELi128ELi64ELi128ELb0ELb0EEELi736EEE", "gram_streamk_glds_batch_kernel"]
ROLLED = "gram_streamk_glds_kernelINS_4TileILi256ELi128ELi64ELi128ELb0ELb0EEELi224EEE"
STEPS = 3                       # k-steps per trip of the main loop
# Instructions that are not MFMAs in the main loop as built: 256 in three k-steps (per k-step 28 LDS reads, 13 loads,
# 16 multiplies, 7 M0 writes, 7 wait states behind them, 6 for the three source pointers, 6 waits, 1 barrier, and the
# loop's own 3 and one wait state over the three).  The cap is that plus two per k-step.
OTHERS_CAP = 256 + 2 * STEPS


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "dopt_kernels.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-w",
                           "-o", str(out), SRC])
    return open(out).read().split("\n")


def _kernel_lines(lines, fragment):
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN6accbpg") and fragment in l.split(":")[0] and ":" in l)
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i])
    return lines[start:end]


def _blocks(body):
    """Basic blocks as lists of opcodes: a block ends in front of a label and behind a branch."""
    blocks, cur = [], []
    for l in body:
        s = l.strip()
        if re.match(r"^\.LBB\d+_\d+:", l):
            blocks.append(cur)
            cur = []
            continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        op = s.split()[0]
        cur.append(op)
        if op.startswith("s_cbranch") or op == "s_branch":
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    return blocks


def _mfmas(block):
    return sum(op.startswith("v_mfma") for op in block)


def _main_loop(lines, fragment):
    return max(_blocks(_kernel_lines(lines, fragment)), key=_mfmas)


def _lds_reads(block):
    return sum(op.startswith("ds_read") for op in block)


@pytest.mark.parametrize("fragment", NEW)
def test_main_loop_is_three_k_steps_without_the_rolled_loops_companions(asm, fragment):
    body = _kernel_lines(asm, fragment)
    scratch = [int(l.split()[-1]) for l in body if ".amdhsa_private_segment_fixed_size" in l]
    assert scratch == [0], (fragment, scratch)
    loop = _main_loop(asm, fragment)
    assert _mfmas(loop) == 128 * STEPS, (fragment, _mfmas(loop))
    assert not [op for op in loop if op.startswith("v_accvgpr") or op.startswith("scratch_")], fragment
    gone = [op for op in loop if op in ("s_mul_i32", "s_cselect_b32", "v_readfirstlane_b32") or re.match(r"v_cmp_\w+_i64", op)]
    assert not gone, (fragment, gone)
    assert loop.count("s_nop") <= 8 * STEPS, (fragment, loop.count("s_nop"))
    # nothing was dropped
    assert loop.count("global_load_lds_dwordx4") == 12 * STEPS and loop.count("global_load_lds_dword") == STEPS, fragment
    assert _lds_reads(loop) == 28 * STEPS, (fragment, _lds_reads(loop))
    assert loop.count("s_barrier") == STEPS, fragment


@pytest.mark.parametrize("fragment", NEW)
def test_fewer_instructions_between_the_mfmas_than_the_rolled_loop(asm, fragment):
    loop, rolled = _main_loop(asm, fragment), _main_loop(asm, ROLLED)
    assert _mfmas(rolled) == 128
    # the rolled loop is the yardstick only while it is the loop it was: same loads and reads per k-step
    assert rolled.count("global_load_lds_dwordx4") == 12 and rolled.count("global_load_lds_dword") == 1
    assert _lds_reads(rolled) == 28
    others, others_rolled = len(loop) - _mfmas(loop), len(rolled) - _mfmas(rolled)
    print("%s: %d instructions that are not MFMAs in %d k-steps; rolled loop %d in one; s_nop %d against %d"
          % (fragment, others, STEPS, others_rolled, loop.count("s_nop"), rolled.count("s_nop")))
    assert others < STEPS * others_rolled, (fragment, others, others_rolled)
    assert others <= OTHERS_CAP, (fragment, others)


@pytest.mark.parametrize("fragment", NEW)
def test_tail_steps_are_whole_k_steps(asm, fragment):
    """The tail is one to four k-steps on stages 0, 1, 2, 0, each a block of its own behind the test that reaches it."""
    blocks = _blocks(_kernel_lines(asm, fragment))
    loop = max(blocks, key=_mfmas)
    tail = [b for b in blocks if b is not loop and _mfmas(b) > 8]       # (the dual tiles' loop runs its MFMAs one to a block)
    assert len(tail) == 4, (fragment, [_mfmas(b) for b in tail])
    for b in tail:
        assert _mfmas(b) == 128, (fragment, _mfmas(b))
        assert not [op for op in b if op.startswith("scratch_")], fragment
        assert b.count("global_load_lds_dwordx4") == 12 and b.count("global_load_lds_dword") == 1, fragment
        assert b.count("s_barrier") == 1, fragment


@pytest.mark.parametrize("fragment", NEW)
def test_compiler_m0_writes_reach_their_loads(asm, fragment):
    """As tests/test_isa_cpu.py has it for the rolled loop: between an M0 write the compiler emitted and the LDS-DMA
    load it belongs to there may be no hand-written load statement (they write M0 themselves; their "m0" clobber is
    what keeps the compiler's own writes from moving across them)."""
    body = [l.strip() for l in _kernel_lines(asm, fragment)]
    in_asm, pending, runs = False, None, 0
    for l in body:
        if l.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if l.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if in_asm:
            if "m0" in l:
                runs += 1
                assert pending is None, "%s: asm statement writes M0 between the compiler's '%s' and its load" % (fragment, pending)
            continue
        if re.match(r"s_\w+\s+m0,", l):
            pending = l
        elif l.startswith("global_load_lds") or l.startswith("buffer_load") and " lds" in l:
            pending = None
    assert runs > 0, "%s: no hand-written load statement found -- the check above tested nothing" % fragment
