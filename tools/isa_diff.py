#!/usr/bin/env python3
"""Compare two device-assembly listings function by function, whichever translation unit a function lives in.
usage: tools/isa_diff.py A B [--show]     A, B: listings of `make -C <pkg>/csrc isa OUT=<file>` (or any hipcc -S output)

Prints one line per symbol -- identical, differs, missing (in A only) or added (in B only) -- and the four totals; --show
adds a unified diff under every symbol that differs.  A function is what stands between its `.type <symbol>,@function`
line and its `End function` line, the kernel descriptor included.  Before two functions are compared their comments are
stripped and their local labels (.LBB<n>_<m>, .Lfunc_end<n>, ...) are renumbered in order of appearance: both carry the
function's ordinal within its unit, which changes when a function moves.  A symbol that occurs twice in one listing is an
error.  Exit status: 0 if every symbol is identical, 1 otherwise."""
import difflib
import re
import sys


def functions(path):
    """{symbol: [normalised lines]} of one listing."""
    out, sym, lines = {}, None, None
    for raw in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", raw)
        if m:
            sym, lines = m.group(1), []
            if sym in out:
                sys.exit(f"{path}: {sym} occurs twice")
        if sym is None:
            continue
        end = "-- End function" in raw
        text = raw.split(";", 1)[0].rstrip()
        if text.strip():
            lines.append(text)
        if end:
            labels = {}
            rename = lambda m: labels.setdefault(m.group(0), f".L{len(labels)}")
            out[sym] = [re.sub(r"\.L[A-Za-z0-9_$]+", rename, l) for l in lines]
            sym = None
    return out


def main(argv):
    show = "--show" in argv
    paths = [a for a in argv if a != "--show"]
    if len(paths) != 2:
        sys.exit(__doc__)
    a, b = functions(paths[0]), functions(paths[1])
    count = {"identical": 0, "differs": 0, "missing": 0, "added": 0}
    for sym in sorted(set(a) | set(b)):
        verdict = "missing" if sym not in b else "added" if sym not in a else "identical" if a[sym] == b[sym] else "differs"
        count[verdict] += 1
        print(f"{verdict:9s} {sym}")
        if show and verdict == "differs":
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a[sym], b[sym], paths[0], paths[1], lineterm="", n=2))
    print(", ".join(f"{n} {k}" for k, n in count.items()), f"({len(a)} symbols in A, {len(b)} in B)")
    return 0 if count["identical"] == len(a) == len(b) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
