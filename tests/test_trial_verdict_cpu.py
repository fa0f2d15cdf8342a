"""The verdict of accbpg_dopt_burg_trial is a pure host function of the trial's status block
(accbpg_and_fw_amd/csrc/trial_verdict.h).  The header is compiled alone with the host compiler, with a small main that
fills status blocks and prints the verdicts: a clean block is OK, every single flag of every stage means REPLAY, and a
compare word that carries the trial's stamp means OK with F[k] not answered.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "trial_verdict.h"
using namespace accbpg;

struct Block {
    double d[TRIAL_DOUBLES];
    Block() {
        memset(d, 0, sizeof(d));
        d[TRIAL_GRAD] = 12.5; d[TRIAL_VALUE] = 12.25;              // log dets
        d[TRIAL_LS] = -0.5; d[TRIAL_LS + 1] = 1e-3; d[TRIAL_LS + 2] = 2e-3; d[TRIAL_LS + 3] = 1e-9;
        pint()[TRIAL_PROX_INFO] = 3; pint()[TRIAL_PROX_INFO + 1] = 7;
    }
    int* eflag(int eval) { return reinterpret_cast<int*>(d + eval + 16); }
    int* pint() { return reinterpret_cast<int*>(d + TRIAL_PROX); }
    int* cmp() { return reinterpret_cast<int*>(d + TRIAL_CMP); }
};

static void show(const char* name, const Block& b, TrialAsked a) {
    const TrialVerdict v = trial_verdict(b.d, a);
    printf("%s replay=%d answered=%d chol=%d prox=%d\n", name, v.replay, v.fk_answered, v.chol_gave_up, v.prox_gave_up);
}

int main() {
    const TrialAsked none = {0, 0}, cmp = {41, 0}, multi = {0, 1}, cmp_multi = {41, 1};
    { Block b; show("clean", b, none); }
    { Block b; b.cmp()[0] = 40; show("clean_answered", b, cmp); }           // an older stamp: x_prev equals the record
    { Block b; b.cmp()[0] = 41; show("clean_mismatch", b, cmp); }           // this trial's stamp: it differs
    { Block b; b.cmp()[0] = 41; show("clean_not_asked", b, none); }
    { Block b; show("clean_multi", b, cmp_multi); }
    const int evals[2] = {TRIAL_GRAD, TRIAL_VALUE};
    const char* en[2] = {"grad", "value"};
    for (int e = 0; e < 2; ++e) {
        { Block b; b.eflag(evals[e])[TRIAL_FLAG_ABORT] = 1; printf("%s_", en[e]); show("abort", b, cmp); }
        { Block b; b.eflag(evals[e])[TRIAL_FLAG_NEG_X] = 1; printf("%s_", en[e]); show("neg_x", b, cmp); }
        { Block b; b.eflag(evals[e])[TRIAL_FLAG_NOT_PD] = 1; printf("%s_", en[e]); show("not_pd", b, cmp); }
    }
    { Block b; b.pint()[TRIAL_FLAG_NONPOS] = 1; show("prox_nonpos", b, cmp); }
    { Block b; b.pint()[TRIAL_PROX_GAVE_UP] = 1; show("prox_gave_up", b, multi); }
    { Block b; b.pint()[TRIAL_PROX_GAVE_UP] = 1; show("prox_word_stale", b, none); }   // single-workgroup form: not written
    { Block b; b.d[TRIAL_LS + 3] = 0.0; show("ls_zero", b, cmp); }
    { Block b; b.d[TRIAL_LS + 3] = -1e-300; show("ls_negative", b, cmp); }
    { Block b; b.d[TRIAL_LS + 3] = NAN; show("ls_nan", b, cmp); }
    printf("layout grad=%d value=%d ls=%d prox=%d cmp=%d doubles=%d eval=%d abort=%d not_pd=%d neg_x=%d nonpos=%d gave_up=%d info=%d\n",
           TRIAL_GRAD, TRIAL_VALUE, TRIAL_LS, TRIAL_PROX, TRIAL_CMP, TRIAL_DOUBLES, TRIAL_EVAL_DOUBLES, TRIAL_FLAG_ABORT,
           TRIAL_FLAG_NOT_PD, TRIAL_FLAG_NEG_X, TRIAL_FLAG_NONPOS, TRIAL_PROX_GAVE_UP, TRIAL_PROX_INFO);
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
def verdicts(tmp_path_factory):
    d = tmp_path_factory.mktemp("verdict")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "verdict"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    table = {}
    for line in out.splitlines():
        name, *fields = line.split()
        table[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return table


def test_clean_block_is_ok(verdicts):
    assert verdicts["clean"] == {"replay": 0, "answered": 0, "chol": 0, "prox": 0}
    assert verdicts["clean_multi"] == {"replay": 0, "answered": 1, "chol": 0, "prox": 0}


def test_compare_word(verdicts):
    """A word that holds anything but this trial's stamp: x_prev equals the record.  The trial's own stamp: it differs,
    which is a clean trial whose F[k] the caller evaluates.  No compare enqueued: never answered."""
    assert verdicts["clean_answered"] == {"replay": 0, "answered": 1, "chol": 0, "prox": 0}
    assert verdicts["clean_mismatch"] == {"replay": 0, "answered": 0, "chol": 0, "prox": 0}
    assert verdicts["clean_not_asked"] == {"replay": 0, "answered": 0, "chol": 0, "prox": 0}


@pytest.mark.parametrize("name", ["grad_abort", "grad_neg_x", "grad_not_pd", "value_abort", "value_neg_x", "value_not_pd",
                                  "prox_nonpos", "prox_gave_up", "ls_zero", "ls_negative", "ls_nan"])
def test_every_single_flag_replays(verdicts, name):
    v = verdicts[name]
    assert v["replay"] == 1
    assert v["answered"] == 0                                   # a replayed trial answers nothing
    assert v["chol"] == (1 if name.endswith("abort") else 0)    # the abandoned factorisation: fall back from now on
    assert v["prox"] == (1 if name == "prox_gave_up" else 0)


def test_give_up_word_counts_only_for_the_multi_workgroup_form(verdicts):
    assert verdicts["prox_word_stale"] == {"replay": 0, "answered": 0, "chol": 0, "prox": 0}


def test_header_stands_alone_and_its_slices_do_not_overlap(verdicts):
    """The header includes nothing but stdint.h (the fixture compiled it with the host compiler alone), and the stages'
    slices of the status block lie one behind the other inside TRIAL_DOUBLES.  That the evaluation slices are laid out
    as the library's own status words is a static_assert in capi.hip, checked whenever the library is built."""
    includes = [ln for ln in open(os.path.join(HEADER_DIR, "trial_verdict.h")) if ln.startswith("#include")]
    assert includes == ["#include <stdint.h>\n"]
    lay = verdicts["layout"]
    assert lay["grad"] + lay["eval"] <= lay["value"] and lay["value"] + lay["eval"] <= lay["ls"]
    assert lay["ls"] + 4 <= lay["prox"] and lay["prox"] + 4 <= lay["cmp"] and lay["cmp"] + 1 <= lay["doubles"]
    assert lay["eval"] == 16 + 8 // 2                           # 16 scalars, then 8 int flags
    assert max(lay["abort"], lay["not_pd"], lay["neg_x"], lay["nonpos"]) < 8 and lay["gave_up"] < 8 and lay["info"] + 1 < 8
