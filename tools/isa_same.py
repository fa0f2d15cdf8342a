"""Do two device assemblies hold the same kernels?

    hipcc <the Makefile's flags> -S --cuda-device-only -o A.s csrc/dopt_kernels.hip      (one commit)
    hipcc <the Makefile's flags> -S --cuda-device-only -o B.s csrc/dopt_kernels.hip      (the other)
    python tools/isa_same.py A.s B.s

Each file is split into kernels, from the kernel's mangled label through its `.end_amdhsa_kernel` (so the kernel
descriptor, the `.amdhsa_*` lines, is part of the compared text).  `;` comments are dropped and the numbers of the
compiler's local labels (.LBB*, .Ltmp*, .Lfunc_*) are blanked, since they count through the whole file.  Every kernel
whose text differs, or that one side lacks, is reported; the exit status is 0 only when there is none.  For a change that
is meant to touch host code alone.  Needs no GPU."""
import re
import sys

LOCAL = re.compile(r"\.(LBB|Ltmp|Lfunc_[a-z]+)[0-9_]+")


def kernels(path):
    """{mangled name: normalised text} of the kernels of one assembly file"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        body = []
        for l in lines[start:end + 1]:
            l = LOCAL.sub(lambda m: "." + m.group(1), l.split(";")[0]).strip()
            if l:
                body.append(l)
        out[name] = body
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in %s: %s" % (sys.argv[2] if name not in a else sys.argv[1], name))
            bad += 1
        elif a[name] != b[name]:
            n = sum(1 for x, y in zip(a[name], b[name]) if x != y) + abs(len(a[name]) - len(b[name]))
            print("differs (%d of %d lines): %s" % (n, len(a[name]), name))
            bad += 1
    print("%d kernels in %s, %d in %s, %d on both sides, %d differ or are missing" %
          (len(a), sys.argv[1], len(b), sys.argv[2], len(set(a) & set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
