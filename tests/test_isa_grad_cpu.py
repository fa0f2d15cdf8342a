"""The gradient kernel's dealt-out k-step is what it claims to be (CPU only: hipcc cross-compiles without a GPU).

Tile::grad_step_dealt (csrc/mfma_tile.hpp) puts at most one part of the fragment reads behind a pair of MFMAs, and a
part is DEALT_PART_VALUES fragment values; the block schedule it replaces (Tile::grad_step) issues the twelve values of
a fragment group in one piece.  In the basic block with the most MFMAs of the production instantiation there are therefore
never more LDS read instructions, nor more values read, between two consecutive MFMAs than a part has values; in the same
loop on the block schedule (COLNORM_CV | 1024, launched by accbpg_debug_grad_variant code 4) twelve values are read between
two MFMAs somewhere, which shows that the count can see a block.  (The compiler pairs neighbouring reads into ds_read2
instructions, so the twelve values of a block are six to twelve instructions; a ds_read2 counts as two values.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc")
SRC = os.path.join(CSRC, "dopt_kernels.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PRODUCTION = "colnorm_glds_kernelINS_4TileILi256ELi128ELi64ELi128ELb1ELb0EEELi256EEE"
BLOCK_SCHEDULE = "colnorm_glds_kernelINS_4TileILi256ELi128ELi64ELi128ELb1ELb0EEELi1280EEE"     # COLNORM_CV | 1024
GROUP_VALUES = 12            # four A rows and eight B columns of a fragment group


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_grad") / "dopt_kernels.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-w",
                           "-o", str(out), SRC])
    return open(out).read().split("\n")


def _part_values():
    """the size of a dealt part, from the source"""
    m = re.search(r"static constexpr int DEALT_PART_VALUES = (\d+);", open(os.path.join(CSRC, "mfma_tile.hpp")).read())
    assert m, "Tile::DEALT_PART_VALUES not found"
    return int(m.group(1))


def _largest_block(lines, fragment):
    """opcodes of the basic block (label to label) with the most MFMAs of the kernel whose mangled name has `fragment`"""
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN6accbpg") and fragment in l.split(":")[0] and ":" in l)
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i])
    blocks, cur = [], []
    for l in lines[start:end]:
        if re.match(r"^\.LBB\d+_\d+:", l):
            blocks.append(cur)
            cur = []
        cur.append(l.strip().split(" ")[0].split("\t")[0] if l.strip() else "")
    blocks.append(cur)
    return max(blocks, key=lambda b: sum(op.startswith("v_mfma") for op in b))


def _reads_between_mfmas(block):
    """(instructions, values) of the LDS reads between each two consecutive MFMAs of the block"""
    gaps, insts, values, seen = [], 0, 0, False
    for op in block:
        if op.startswith("v_mfma"):
            if seen:
                gaps.append((insts, values))
            seen, insts, values = True, 0, 0
        elif op.startswith("ds_read"):
            insts += 1
            values += 2 if op.startswith("ds_read2") else 1
    return gaps


def test_production_deals_its_reads_out(asm):
    part = _part_values()
    assert part == 2                                             # a part of read_part_g is two fragment values
    block = _largest_block(asm, PRODUCTION)
    gaps = _reads_between_mfmas(block)
    assert len(gaps) >= 127, len(gaps)
    print("production: %d MFMAs, most read instructions / values between two: %d / %d, reads in all: %d"
          % (len(gaps) + 1, max(g[0] for g in gaps), max(g[1] for g in gaps), sum(g[1] for g in gaps)))
    assert max(g[0] for g in gaps) <= part and max(g[1] for g in gaps) <= part
    # the reads are there at all: four groups of twelve values, dealt between the MFMAs
    assert sum(g[1] for g in gaps) >= 4 * GROUP_VALUES - part


def test_block_schedule_is_seen_as_blocks(asm):
    block = _largest_block(asm, BLOCK_SCHEDULE)
    gaps = _reads_between_mfmas(block)
    assert len(gaps) >= 127, len(gaps)
    print("block schedule: %d MFMAs, most read instructions / values between two: %d / %d"
          % (len(gaps) + 1, max(g[0] for g in gaps), max(g[1] for g in gaps)))
    assert max(g[1] for g in gaps) >= GROUP_VALUES
