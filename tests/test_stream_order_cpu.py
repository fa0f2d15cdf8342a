"""Source lint: every device fill or copy of the library names a stream.

A fill without a stream goes to the null stream, and a non-blocking stream -- every stream the package works on -- does
not wait for the null stream: a handle created or first used there could start before its cleared state had landed.
So in accbpg_and_fw_amd/csrc no call of a stream-less hipMemset form is allowed, every asynchronous fill or copy must
pass a stream that is not a literal null, and the blocking hipMemcpy calls that remain (they complete before they
return) are listed here one by one, by file and by what they write."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc")

NO_STREAM_FILLS = ("hipMemset", "hipMemsetD8", "hipMemsetD16", "hipMemsetD32", "hipMemset2D", "hipMemset3D")
NULL_STREAMS = ("0", "NULL", "nullptr")

# blocking host-to-device uploads in create (and the debug allocator's band copies): (file, destination) -> what it is
BLOCKING_COPIES = {
    ("dopt_kernels.hip", "*dev"): "upload(): the plan tables of build_plans (tiles, wg_ranges, gram_cstart, gram_contrib, "
                                  "ops, red, chol_jobs)",
    ("batch.hip", "b->table"): "per-instance pointers of a fused batch",
    ("batch.hip", "b->chol_table[0]"): "Cholesky arguments of a fused batch, value form",
    ("batch.hip", "b->chol_table[1]"): "Cholesky arguments of a fused batch, gradient form",
    ("batch.hip", "b->ops_all"): "merge products of all instances",
    ("batch.hip", "b->red_all"): "merge reductions of all instances",
    ("fw_kernels.hip", "b->fw_table"): "per-instance Frank-Wolfe state pointers of a batch",
    ("fw_kernels.hip", "b->fw_div_table"): "per-instance Bregman-step state pointers of a batch",
    ("guard_alloc.hip", "dst"): "raw_upload / raw_download of the debug guard bands (a debug switch, off by default)",
}


def strip_comments(text):
    """C++ source without // and /* */ comments; string and character literals are kept as they are."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        elif text.startswith("//", i):
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            out.append(" " + "\n" * text.count("\n", i, n if j < 0 else j))
            i = n if j < 0 else j + 2
        else:
            out.append(c)
            i += 1
    return "".join(out)


def calls(code, pattern):
    """(name, [arguments], line) of every call whose name matches `pattern` in comment-free code."""
    for mt in re.finditer(r"\b(%s)\s*\(" % pattern, code):
        depth, args, start, i = 1, [], mt.end(), mt.end()
        while i < len(code) and depth:
            c = code[i]
            if c in "([{":
                depth += 1
            elif c in ")]}":
                depth -= 1
                if depth == 0:
                    args.append(code[start:i])
            elif c == "," and depth == 1:
                args.append(code[start:i])
                start = i + 1
            i += 1
        yield mt.group(1), [" ".join(a.split()) for a in args], code.count("\n", 0, mt.start()) + 1


def violations(fname, text):
    """The stream-order violations of one source file, as messages."""
    code = strip_comments(text)
    bad, seen = [], set()
    for name, args, line in calls(code, r"hipMem(?:set|cpy)\w*"):
        where = "%s:%d: %s(%s)" % (fname, line, name, ", ".join(args))
        if name in NO_STREAM_FILLS:
            bad.append(where + " -- a fill without a stream goes to the null stream")
        elif name.endswith("Async"):
            last = re.sub(r"^\(\s*hipStream_t\s*\)\s*", "", args[-1]) if args else ""
            if last in NULL_STREAMS:
                bad.append(where + " -- the stream is a literal null")
        elif name.startswith("hipMemcpy"):
            key = (fname, args[0] if args else "")
            seen.add(key)
            if key not in BLOCKING_COPIES:
                bad.append(where + " -- a blocking copy that is not on the allow-list")
    return bad, seen


def sources():
    files = []
    for ext in ("*.hip", "*.hpp", "*.h"):
        files += glob.glob(os.path.join(CSRC, ext))
    return sorted(files)


def test_the_lint_sees_what_it_should():
    text = """
    // hipMemset(a, 0, n);   a comment does not count
    /* hipMemsetAsync(a, 0, n, 0); nor this */
    void f() {
        hipMemset(p, 0, n);
        ACC_HIP(hipMemsetD32(p, 0, n));
        hipMemsetAsync(p, 0, g(n, 2), 0);
        hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, nullptr);
        hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, (hipStream_t)0);
        hipMemcpy2DAsync(d, 8, s, 8, 8, m, hipMemcpyDeviceToDevice, NULL);
        hipMemsetAsync(p, 0, n, h->stream);
        hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, s0);
        hipMemcpy(q, host, n, hipMemcpyHostToDevice);
        const char* msg = "hipMemset(x, 0, 1) in a string is kept, and found";
    }
    """
    bad, _ = violations("x.hip", text)
    assert len(bad) == 8, bad
    assert [int(b.split(":")[1]) for b in bad] == [5, 6, 7, 8, 9, 10, 13, 14]
    assert sum("without a stream" in b for b in bad) == 3 and sum("literal null" in b for b in bad) == 4
    assert sum("allow-list" in b for b in bad) == 1


def test_every_device_fill_and_copy_names_a_stream():
    files = sources()
    assert len(files) >= 20, files
    bad, seen = [], set()
    for path in files:
        with open(path) as fh:
            b, s = violations(os.path.basename(path), fh.read())
        bad += b
        seen |= s
    assert not bad, "\n" + "\n".join(bad)
    stale = sorted(set(BLOCKING_COPIES) - seen)
    assert not stale, "allow-list entries that no longer exist: %s" % stale
