"""Resources of the one-launch Cholesky kernel (CPU only: hipcc cross-compiles without a GPU).

chol_tiles_kernel needs all its workgroups resident at once, two per CU: that holds only while a workgroup asks for no
more LDS than CT_LDS_BYTES (76 416 bytes: two of them fit the 160 KiB of a CU), no more than 256 registers per lane in
both register files together, and no scratch.  A change to the chain's panel solve that lengthens a live range shows
here before it shows as a launch that no longer fits the chip."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc", "dopt_kernels.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

CT_LDS_BYTES = 76416            # what the kernel asked for when the two-per-CU residency was planned
CT_STATIC_LDS_BYTES = 256       # ... and the most static LDS it ever had beside that
CU_LDS_BYTES = 160 * 1024


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_chol") / "dopt_kernels.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-w",
                           "-o", str(out), SRC])
    lines = open(out).read().split("\n")
    start = next(i for i, l in enumerate(lines)
                 if l.startswith("_ZN6accbpg") and "chol_tiles_kernel" in l.split(":")[0] and ":" in l)
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i])
    return lines[start:end]


def _directive(body, name):
    vals = [int(l.split()[-1]) for l in body if l.strip().startswith(name + " ")]
    assert len(vals) == 1, (name, vals)
    return vals[0]


def test_no_scratch(kernel):
    assert _directive(kernel, ".amdhsa_private_segment_fixed_size") == 0
    assert not [l for l in kernel if l.strip().startswith("scratch_")]


def test_registers_fit_two_workgroups_per_cu(kernel):
    # gfx90a and later: one unified file; next_free_vgpr counts the vector registers up to accum_offset and the
    # accumulation registers behind it
    total = _directive(kernel, ".amdhsa_next_free_vgpr")
    assert total <= 256, total
    assert _directive(kernel, ".amdhsa_accum_offset") <= 256


def test_lds_request_is_ct_lds_bytes(kernel):
    """What a workgroup gets is the dynamic size of its launches plus the kernel's static LDS (256 bytes while it
    voted through the device library's workgroup reduction, none since).  Every launch (through ACC_LAUNCH_LDS, which
    raises the kernel's limit to what the launch asks for) and the limit raised at handle creation, ahead of the
    occupancy query, pass CT_LDS_BYTES, whose value is that of the constants in the source; the static part has not
    grown."""
    src = open(SRC).read()
    const = {}
    for text in (open(os.path.join(os.path.dirname(SRC), "dopt_plan.hpp")).read(), src):
        for name, expr in re.findall(r"constexpr int (NB|SQ|POTRF_TB|CT_LDS_DOUBLES|CT_LDS_BYTES) = ([^;]+);", text):
            const[name] = eval(expr, {"__builtins__": {}}, dict(const))
    assert const["CT_LDS_BYTES"] == CT_LDS_BYTES, const
    assert not re.search(r"chol_tiles_kernel\s*<<<", src)          # no launch beside the ones counted here
    launches = re.findall(r"ACC_LAUNCH_LDS\([^,]+, chol_tiles_kernel,.*?NTHREADS,\s*(\w+),", src)
    assert len(launches) >= 2 and set(launches) == {"CT_LDS_BYTES"}, launches
    assert re.search(r"ensure_lds\(h->device, [^;]*\(chol_tiles_kernel\), CT_LDS_BYTES\)\);\s*int per_cu = 0;\s*"
                     r"ACC_HIP\(hipOccupancyMaxActiveBlocksPerMultiprocessor\(&per_cu, chol_tiles_kernel, NTHREADS, CT_LDS_BYTES\)\)", src)
    static = _directive(kernel, ".amdhsa_group_segment_fixed_size")
    assert static <= CT_STATIC_LDS_BYTES, static
    assert 2 * (const["CT_LDS_BYTES"] + static) <= CU_LDS_BYTES
