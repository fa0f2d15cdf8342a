"""The guard-band registry of the library's device allocator is pure host logic
(accbpg_and_fw_amd/csrc/guard_alloc.hpp): where the user pointer lies in a banded allocation, which bytes are band,
the lookup of acc_free, the comparison of the bands.  The header is compiled alone with the host compiler and a small
main that hands it malloc / free / memcpy as the raw operations, and that program runs stand-alone under the address
and undefined-behaviour sanitizers: a band that the registry itself fills or reads one byte too far is an error there.
The same file checks that no translation unit but the allocator's names hipMalloc / hipFree.  No GPU, nothing loaded
into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc")

MAIN = r"""
#include "guard_alloc.hpp"
#include <stdlib.h>
using namespace accbpg::guard;

static int raw_alloc(void** p, size_t bytes) {
    // page-aligned like the device allocator, and exactly `bytes` long: the sanitizer sees every byte past the layout
    *p = bytes ? aligned_alloc(PAGE, round_up(bytes, PAGE)) : nullptr;
    if (bytes && !*p) return 2;
    return 0;
}
static int raw_release(void* p) { free(p); return 0; }
static int raw_copy(void* d, const void* s, size_t n) { memcpy(d, s, n); return 0; }

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int expect_clean(Registry& r, long long live) {
    int64_t o[3]; Damage d;
    CHECK(r.check(o, &d) == 0);
    CHECK(o[0] == live && o[1] == 0 && o[2] == 0 && !d.any);
    return 0;
}

int main() {
    Registry r(RawOps{raw_alloc, raw_release, raw_copy, raw_copy});
    const size_t sizes[] = {1, 8, 4095, 4096, 4097};
    const size_t B = 8192;

    // the switch: off at first, multiples of 4096 only
    CHECK(r.band() == 0);
    CHECK(r.set_band(100) == -1 && r.set_band(-4096) == -1 && r.band() == 0);
    void* plain[5];
    for (int i = 0; i < 5; ++i) { CHECK(r.allocate(&plain[i], sizes[i], "plain") == 0); memset(plain[i], 0x11, sizes[i]); }
    CHECK(r.live() == 0);
    CHECK(expect_clean(r, 0) == 0);

    // layout arithmetic
    for (size_t s : sizes) {
        const Layout l = layout(s, B);
        CHECK(l.front == B && l.back >= B && l.back < B + PAGE);
        CHECK(l.total == l.front + s + l.back && l.total % PAGE == 0);
        CHECK((l.front + s + l.back) == 2 * B + round_up(s, PAGE));
        printf("layout %zu: front %zu back %zu total %zu\n", s, l.front, l.back, l.total);
    }
    for (size_t o = 0; o < 16; ++o) CHECK(pattern_byte(o) == (unsigned char)(SENTINEL >> (8 * (o % 8))));

    // banded allocations: alignment, bands filled, user region writable end to end
    CHECK(r.set_band((int64_t)B) == 0);
    void* banded[5];
    for (int i = 0; i < 5; ++i) {
        CHECK(r.allocate(&banded[i], sizes[i], i == 2 ? "odd4095" : "banded") == 0);
        CHECK(((uintptr_t)banded[i]) % PAGE == 0);
        const unsigned char* u = (const unsigned char*)banded[i];
        const Layout l = layout(sizes[i], B);
        for (size_t k = 0; k < l.front; ++k) CHECK(*(u - l.front + k) == pattern_byte(k));
        for (size_t k = 0; k < l.back; ++k) CHECK(u[sizes[i] + k] == pattern_byte(l.front + sizes[i] + k));
        uint64_t w; memcpy(&w, u - 8, 8); CHECK(w == SENTINEL);
        memset(banded[i], 0x22, sizes[i]);
    }
    CHECK(r.live() == 5);
    CHECK(expect_clean(r, 5) == 0);
    // a zero-byte request is the raw allocator's
    void* none = (void*)1;
    CHECK(r.allocate(&none, 0, "none") == 0 && none == nullptr && r.live() == 5);

    // damage: in front of, behind, and at the very last byte of a band
    struct Hit { int which; long long at; Side side; long long offset; } hits[] = {
        {2, -1, FRONT, -1},                                         // the byte in front of the user pointer
        {2, -(long long)B, FRONT, -(long long)B},                   // the first byte of the front band
        {2, 4095, BACK, 0},                                         // the first byte behind 4095 user bytes
        {2, 4095 + (long long)B, BACK, (long long)B},               // the last byte of the back band (B + 1 bytes long)
        {4, 4097 + (long long)B + 4094, BACK, (long long)B + 4094}, // ... of the longest back band
        {0, 1, BACK, 0},
    };
    for (const Hit& h : hits) {
        unsigned char* at = (unsigned char*)banded[h.which] + h.at;
        const unsigned char keep = *at;
        *at = (unsigned char)~keep;
        int64_t o[3]; Damage d;
        CHECK(r.check(o, &d) == 0);
        CHECK(o[0] == 5 && o[1] == 1 && o[2] == 1 && d.any);
        CHECK(d.side == h.side && d.offset == h.offset);
        CHECK(d.label == (h.which == 2 ? "odd4095" : "banded"));
        printf("report: %s\n", Registry::describe(d).c_str());
        *at = keep;
        CHECK(expect_clean(r, 5) == 0);
    }
    {   // two bands of one allocation, three bytes
        unsigned char* u = (unsigned char*)banded[3];
        u[-8] ^= 0xFF; u[-7] ^= 0xFF; u[4096 + 17] ^= 0xFF;
        int64_t o[3]; Damage d;
        CHECK(r.check(o, &d) == 0);
        CHECK(o[1] == 2 && o[2] == 3 && d.side == FRONT && d.offset == -8);
        u[-8] ^= 0xFF; u[-7] ^= 0xFF; u[4096 + 17] ^= 0xFF;
    }

    // free in any order, banded and unbanded mixed, with the switch on and off; allocations made meanwhile
    CHECK(r.release(banded[1]) == 0 && r.live() == 4);
    CHECK(r.release(plain[3]) == 0 && r.live() == 4);
    CHECK(r.set_band(0) == 0);
    void* late = nullptr;
    CHECK(r.allocate(&late, 100, "late") == 0 && r.live() == 4);
    CHECK(r.release(banded[4]) == 0 && r.live() == 3);
    CHECK(expect_clean(r, 3) == 0);
    CHECK(r.release(plain[0]) == 0 && r.release(banded[0]) == 0 && r.release(late) == 0);
    CHECK(r.set_band(2 * (int64_t)B) == 0);
    void* wide = nullptr;
    CHECK(r.allocate(&wide, 24, "wide") == 0 && r.live() == 3);
    CHECK(r.release(banded[3]) == 0 && r.release(plain[4]) == 0 && r.release(wide) == 0 && r.release(banded[2]) == 0);
    CHECK(r.release(plain[1]) == 0 && r.release(plain[2]) == 0 && r.release(nullptr) == 0);
    CHECK(r.live() == 0);
    CHECK(expect_clean(r, 0) == 0);
    printf("guard ok\n");
    return 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(rocm), "no host C++ compiler found"
    return rocm


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("guard")
    (d / "main.cpp").write_text(MAIN)
    exe = d / "guard"
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, str(d / "main.cpp"), "-o", str(exe)]
    # the sanitizer runtimes linked into the program itself where the compiler knows the switches (gcc; clang's default)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.DEVNULL,
                      stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.check_call(cmd)
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    return run.stdout


def test_header_stands_alone():
    text = open(os.path.join(CSRC, "guard_alloc.hpp")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i or i == "internal.h"], includes


def test_registry_under_host_sanitizers(program_output):
    assert program_output.rstrip().endswith("guard ok"), program_output
    assert "runtime error" not in program_output and "AddressSanitizer" not in program_output


def test_layout_of_the_issue_sizes(program_output):
    got = dict()
    for size, front, back, total in re.findall(r"layout (\d+): front (\d+) back (\d+) total (\d+)", program_output):
        got[int(size)] = (int(front), int(back), int(total))
    assert got == {1: (8192, 8192 + 4095, 20480), 8: (8192, 8192 + 4088, 20480),
                   4095: (8192, 8193, 20480), 4096: (8192, 8192, 20480), 4097: (8192, 8192 + 4095, 24576)}


def test_damage_reports_name_label_side_and_offset(program_output):
    reports = re.findall(r"report: (.*)", program_output)
    assert reports == [
        "guard band damaged: odd4095, front, byte -1 from the user region's start",
        "guard band damaged: odd4095, front, byte -8192 from the user region's start",
        "guard band damaged: odd4095, back, byte +0 from the user region's end",
        "guard band damaged: odd4095, back, byte +8192 from the user region's end",
        "guard band damaged: banded, back, byte +12286 from the user region's end",
        "guard band damaged: banded, back, byte +0 from the user region's end",
    ]


def test_no_bare_device_allocation_outside_the_allocator():
    """Every device buffer of the library comes from acc_malloc and goes back through acc_free, so that the guard bands
    reach it.  (hipHostMalloc / hipHostFree, the pinned host memory, are not meant.)"""
    bare = re.compile(r"(?<![A-Za-z_])hip(Malloc|Free)\s*\(")
    found = []
    names = sorted(os.listdir(CSRC))
    assert "guard_alloc.hip" in names
    for name in names:
        path = os.path.join(CSRC, name)
        if name == "guard_alloc.hip" or not os.path.isfile(path) or not name.endswith((".hip", ".h", ".hpp", ".cpp")):
            continue
        for no, line in enumerate(open(path), 1):
            if bare.search(line):
                found.append("%s:%d: %s" % (name, no, line.strip()))
    assert not found, "\n".join(found)
    assert bare.search(open(os.path.join(CSRC, "guard_alloc.hip")).read())      # (the pattern does find them)
