"""Record the launch plans of build_plans() as a commit had it, for tests/test_plan_cpu.py.

    python tools/gen_plan_golden.py REV [out.npz]

Takes the text of build_plans from `git show REV:accbpg_and_fw_amd/csrc/dopt_kernels.hip`, wraps it in a stand-in
handle struct and host stubs of the HIP calls it makes (hipMalloc allocates on the host, the copies are memcpy, the
attribute and occupancy calls are answered without a device), compiles that with the host compiler, runs it over the
shape table of tests/plan_cases.py and writes the arrays.  Needs no GPU.  It works for the commits in which build_plans
is one self-contained function, that is up to the commit before csrc/dopt_plan.hpp: tests/golden/dopt_plans_parent.npz
was written from that commit, so the header's planners are held to what the function gave before it was taken apart."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plan_cases as P  # noqa: E402

PREAMBLE = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0 };
enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToDevice = 3 };
enum { ACCBPG_OK = 0, ACCBPG_ERR_ARG = 1, ACCBPG_ERR_HIP = 2 };
#define ACC_HIP(call) do { if ((call) != hipSuccess) return ACCBPG_ERR_HIP; } while (0)
#define ACC_TRY(call) do { int rc__ = (call); if (rc__ != ACCBPG_OK) return rc__; } while (0)
// tables are allocated for real (they are read back below); the big buffers get addresses that are never touched
static uintptr_t g_fake = (uintptr_t)1 << 44;
template <class T>
static hipError_t hipMalloc(T** p, size_t bytes) {
    if (bytes <= ((size_t)1 << 20)) { *p = (T*)calloc(bytes ? bytes : 1, 1); return hipSuccess; }
    *p = (T*)g_fake;
    g_fake += (bytes + 4095) / 4096 * 4096 + 4096;
    return hipSuccess;
}
static hipError_t hipMemcpy(void* d, const void* s, size_t bytes, int) { memcpy(d, s, bytes); return hipSuccess; }
template <class... A> static hipError_t hipMemcpy2DAsync(A...) { return hipSuccess; }
template <class... A> static hipError_t hipMemset(A...) { return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static hipError_t hipGetLastError() { return hipSuccess; }
#define set_lds(...) ACCBPG_OK
static int set_lds_gemm_ops() { return ACCBPG_OK; }
#define hipOccupancyMaxActiveBlocksPerMultiprocessor(p, ...) (*(p) = 2, hipSuccess)    /* two workgroups per CU */

struct GemmOp { const double* A; const double* B; double* C; int64_t lda, ldb, ldc; int32_t M, N, K, lower_only, tri, koff; double alpha, beta; };
struct RedOp { double* C; const double* P; int64_t ldc; int32_t M, N, ns, pad; };
struct TileRC { int32_t rb, cb; int32_t d1 = -1, d2 = -1; };
struct CholJob { int i, j; };
constexpr int BK = 16, NB = 64, GRAM_RMAX = 4, CT_TMAX = 32, NTHREADS = 256, CT_AUX = 1, CT_LDS_BYTES = 0;
template <bool BKM, bool EDGE = true> struct TileBig { static constexpr int BM = 256, BN = 128; };
template <bool BKM, bool EDGE = true> struct TileSmall { static constexpr int BM = 64, BN = 64; };
static int g_plan_flags = 0;
struct accbpg_dopt {
    const double* V = nullptr;
    int64_t m = 0, n = 0, ldv = 0;
    hipStream_t stream = nullptr;
    int num_cu = 256;
    bool big = false, vec_ok = false, use_glds = true, has_duals = false;
    int gram_grid_cap = 0;
    double *Lbuf = nullptr, *Wbuf = nullptr, *Tbuf = nullptr, *slabs = nullptr, *Vblk = nullptr, *Pbuf = nullptr, *Gbuf = nullptr;
    TileRC* tiles = nullptr;
    int64_t* wg_ranges = nullptr;
    int32_t *gram_cstart = nullptr, *gram_contrib = nullptr;
    int ntiles = 0, gram_grid = 0, gram_per = 0, gram_nslot = 2, gram_chunks = 1;
    int64_t kiters = 0, gram_nc = 0;
    GemmOp *ops = nullptr, *chol_op = nullptr;
    RedOp* red = nullptr;
    std::vector<GemmOp> ops_host;
    std::vector<RedOp> red_host;
    struct MergeStage { int kind, begin, end, maxm, maxn; };
    std::vector<MergeStage> merge_stages;
    bool chol_tiles_ok = false;
    int chol_tiles_grid = 0, chol_slots = 0;
    void* chol_jobs = nullptr;
    int* chol_ready = nullptr;
    double *chol_aux = nullptr, *chol_hand = nullptr;
};
"""

MAIN = r"""
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    Case c;
    while (read_case(f, &c)) {
        accbpg_dopt h;
        const long long mm = c.m * c.m;
        h.m = c.m; h.n = c.n; h.ldv = c.ldv; h.big = c.big; h.vec_ok = c.vec_ok; h.use_glds = c.use_glds;
        h.num_cu = c.num_cu; h.gram_grid_cap = c.grid_cap;
        g_plan_flags = c.flags;
        h.V = (const double*)((uintptr_t)1 << 40);
        h.Lbuf = (double*)((uintptr_t)2 << 40); h.Wbuf = (double*)((uintptr_t)3 << 40); h.Tbuf = (double*)((uintptr_t)4 << 40);
        const int rc = build_plans(&h);
        if (rc != ACCBPG_OK) { fprintf(stderr, "build_plans(%s) -> %d\n", c.name, rc); return 1; }
        printf("case %s\n", c.name);
        if (!strcmp(c.kind, "gram")) {
            dump_scalar("chunks", h.gram_chunks); dump_scalar("nc", h.gram_nc); dump_scalar("want_block_copy", h.Vblk != nullptr);
            dump_scalar("kiters", h.kiters); dump_scalar("has_duals", h.has_duals); dump_scalar("ntiles", h.ntiles);
            dump_scalar("grid", h.gram_grid); dump_scalar("per", h.gram_per); dump_scalar("nslot", h.gram_nslot);
            dump_array("tiles", (const int32_t*)h.tiles, (size_t)h.ntiles * 4);
            dump_array("ranges", h.wg_ranges, (size_t)h.gram_grid * GRAM_RMAX * 2);
            dump_array("cstart", h.gram_cstart, (size_t)h.ntiles * 2 + 1);
            const size_t pairs = (size_t)h.gram_cstart[(size_t)h.ntiles * 2];
            dump_array("contrib", h.gram_contrib, pairs ? pairs * 2 : 1);
        } else {
            const Bases bs = {{h.Lbuf, h.Wbuf, h.Tbuf, h.Pbuf}, mm};
            dump_merges(bs, h.ops_host.data(), h.ops_host.size(), h.red_host.data(), h.red_host.size(), h.merge_stages.data(),
                        h.merge_stages.size(), (const CholJob*)h.chol_jobs, h.chol_tiles_ok ? (size_t)h.chol_tiles_grid : 0);
        }
    }
    return 0;
}
"""


def compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")


def build_plans_text(rev):
    src = subprocess.check_output(["git", "-C", ROOT, "show", "%s:accbpg_and_fw_amd/csrc/dopt_kernels.hip" % rev], text=True)
    lines = src.split("\n")
    start = lines.index("int build_plans(accbpg_dopt* h) {")
    end = next(i for i in range(start, len(lines)) if lines[i] == "}")
    text = "\n".join(lines[start:end + 1])
    if "plan_gram(" in text:
        sys.exit("build_plans of %s already plans through csrc/dopt_plan.hpp: nothing to take apart" % rev)
    return text


def main():
    rev = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "dopt_plans_parent.npz")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "main.cpp"), "w") as f:
            f.write(PREAMBLE + P.DUMP_CPP + build_plans_text(rev) + MAIN)
        with open(os.path.join(d, "cases.txt"), "w") as f:
            f.write(P.cases_text())
        exe = os.path.join(d, "plans")
        subprocess.check_call([compiler(), "-std=c++17", "-O1", "-w", os.path.join(d, "main.cpp"), "-o", exe])
        text = subprocess.check_output([exe, os.path.join(d, "cases.txt")], text=True)
    rec = P.pack(P.parse(text))
    rec["rev"] = np.array(subprocess.check_output(["git", "-C", ROOT, "rev-parse", rev], text=True).strip())
    np.savez_compressed(out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out, len(rec), os.path.getsize(out)))


if __name__ == "__main__":
    main()
