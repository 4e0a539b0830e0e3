#!/usr/bin/env python3
"""dev tool: are two device listings (hipcc <the Makefile's flags> --cuda-device-only -S x.hip) the same code?

    python tools/device_listing_diff.py A.s B.s [A2.s B2.s ...]

For a host-only change they must be.  Every __hip_cuid_<hash> is replaced by one word first.  Prints "identical" where the
files then agree byte for byte; otherwise compares kernel by kernel (a moved template instantiation reorders whole kernels
and renumbers their local labels, nothing else): "same kernels, other order", or the kernels that exist on one side only or
differ.  Exit status 1 unless every pair is the same code.
"""
import re
import sys

BEGIN = re.compile(r'^\t\.section\t\.text\.(\S+?),.*\n\t\.(?:globl|weak)\t\1\b', re.M)


def kernels(path):
    s = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    meta = s.index("\t.amdgpu_metadata")
    tail = s.index("\t.section\t.AMDGPU.gpr_maximums", 0, meta)       # behind the last kernel
    cuts = [m.start() for m in BEGIN.finditer(s, 0, tail)] + [tail]
    parts = {"": s[:cuts[0]] + s[tail:meta]}
    for a, b in zip(cuts, cuts[1:]):
        # the function's number in its local labels (.LBB12_3, .Lfunc_end12) and in the comments that name them (BB12_3),
        # and the padding in front of a comment, which follows the label's length
        body = re.sub(r"(\.LBB|\bBB|\.Lfunc_end|\.Lfunc_begin|\.Ltmp)\d+", r"\1", s[a:b])
        parts[BEGIN.match(s, a).group(1)] = re.sub(r" +;", " ;", body)
    head, foot = s[meta:].split("amdhsa.kernels:\n", 1)[0], s[s.index("\namdhsa.target:", meta) + 1:]
    parts["metadata frame"] = head + foot
    entries = s[meta + len(head):len(s) - len(foot)]
    for entry in re.split(r"^  - (?=\.agpr_count)", entries, flags=re.M)[1:]:      # one metadata entry per kernel
        parts["metadata " + re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)] = entry
    return s, parts


def main(argv):
    bad = 0
    for a, b in zip(argv[0::2], argv[1::2]):
        (sa, pa), (sb, pb) = kernels(a), kernels(b)
        if sa == sb:
            print("%s: identical" % b)
            continue
        diff = sorted(k for k in set(pa) | set(pb) if pa.get(k) != pb.get(k))
        if not diff:
            print("%s: same %d kernels, other order" % (b, sum(1 for k in pa if k and not k.startswith("metadata "))))
            continue
        bad = 1
        for k in diff:
            print("%s: %s %s" % (b, "only in the first:" if k not in pb else ("only in the second:" if k not in pa else "differs:"), k or "(header)"))
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
