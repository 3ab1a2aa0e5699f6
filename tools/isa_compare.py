#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files (hipcc -S), CPU only.

    python tools/isa_compare.py OLD.s NEW.s

For every kernel symbol of either file one line is printed:

    <class>  <instructions old>  <instructions new>  <differing lines>  <symbol>

identical   the normalised bodies are equal line for line;
equivalent  equal instruction counts, equal multisets of mnemonics over every
            non-scalar instruction (everything not starting with s_) and equal
            values of the compiler's resource comments (VGPRs, AGPRs, SGPRs,
            scratch, LDS, occupancy): the compiler renamed registers, swapped
            independent instructions or laid a block out the other way round;
changed     anything else, a kernel present in one file only included.

A kernel whose six resource comments were not all found is never `equivalent`.
`identical` asks only that the bodies and whatever resource comments were found
be equal: equal bodies need no second witness.

A body runs from the symbol's label to its .Lfunc_end label (a role-specialised
kernel ends more than once, so the first s_endpgm is not the end).  Comments
are stripped, blank lines dropped, and local labels renumbered in order of
appearance.  The tool parses; it looks for no particular instruction.
Exit status: 0 when no kernel is `changed`, else 1.
"""
import collections
import difflib
import re
import sys

# the compiler's resource comments after a kernel, by the name they are compared under
RESOURCES = {"NumVgprs": "VGPRs", "NumAgprs": "AGPRs", "NumSgprs": "SGPRs", "TotalNumSgprs": "SGPRs",
             "ScratchSize": "scratch", "LDSByteSize": "LDS", "Occupancy": "occupancy"}
_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)*")
_SYMBOL = re.compile(r"^([A-Za-z_][\w$.]*):")


def _strip(line):
    return line.split(";", 1)[0].rstrip()


def kernels(text):
    """{symbol: (body lines as written, {resource: value})} of every kernel.
    A kernel is a symbol with a .Lfunc_end label after it and an s_endpgm in
    between; its resource comments follow the .Lfunc_end label."""
    lines = text.split("\n")
    res = {}
    i = 0
    while i < len(lines):
        m = _SYMBOL.match(lines[i])
        if not m:
            i += 1
            continue
        end = next((j for j in range(i + 1, len(lines)) if lines[j].startswith(".Lfunc_end")), None)
        nxt = next((j for j in range(i + 1, len(lines)) if _SYMBOL.match(lines[j])), len(lines))
        if end is None or end > nxt:
            i += 1
            continue
        body = lines[i + 1:end]
        if any(_strip(l).strip() == "s_endpgm" for l in body):
            tail = lines[end:nxt]
            rsrc = {}
            for l in tail:
                r = re.match(r"^\s*;\s*(\w+):\s*(\d+)\b", l)
                if r and r.group(1) in RESOURCES:
                    rsrc[RESOURCES[r.group(1)]] = int(r.group(2))
            res[m.group(1)] = (body, rsrc)
        i = end + 1
    return res


def normalise(body):
    """comments and blank lines out, local labels renumbered in order of appearance"""
    names = {}

    def rename(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))

    out = []
    for l in body:
        l = _strip(l).strip()
        if l:
            out.append(_LABEL.sub(rename, re.sub(r"\s+", " ", l)))
    return out


def instructions(norm):
    """the instruction lines of a normalised body: no labels, no directives"""
    return [l for l in norm if not l.endswith(":") and not l.startswith(".")]


def classify(old, new):
    """(class, instructions old, instructions new, differing lines) for two
    kernels (body, resources), either of which may be None"""
    if old is None or new is None:
        k = old or new
        n = len(instructions(normalise(k[0])))
        return ("changed", n if old else 0, n if new else 0, n)
    a, b = normalise(old[0]), normalise(new[0])
    ia, ib = instructions(a), instructions(b)
    if a == b and old[1] == new[1]:
        return ("identical", len(ia), len(ib), 0)
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    differing = max(len(a), len(b)) - sum(blk.size for blk in sm.get_matching_blocks())

    def vector_mix(ins):
        return collections.Counter(l.split(" ", 1)[0] for l in ins if not l.startswith("s_"))

    complete = set(old[1]) == set(RESOURCES.values())  # a kernel whose comments were not found is never equivalent
    same = len(ia) == len(ib) and vector_mix(ia) == vector_mix(ib) and old[1] == new[1] and complete
    return ("equivalent" if same else "changed", len(ia), len(ib), differing)


def compare(old_text, new_text):
    """[(symbol, class, instructions old, instructions new, differing lines)]"""
    ko, kn = kernels(old_text), kernels(new_text)
    return [(s,) + classify(ko.get(s), kn.get(s)) for s in sorted(set(ko) | set(kn))]


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    with open(argv[1]) as f:
        old = f.read()
    with open(argv[2]) as f:
        new = f.read()
    rows = compare(old, new)
    for sym, cls, n_old, n_new, diff in rows:
        print("%-10s %7d %7d %5d  %s" % (cls, n_old, n_new, diff, sym))
    return 1 if any(r[1] == "changed" for r in rows) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
