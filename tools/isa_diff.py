"""Per-function text comparison of hipcc -S (gfx950) assembly files: has a
kernel's code changed between two builds, whichever translation unit emits it?

    python tools/isa_diff.py A.s B.s [MORE_B.s ...]

A is one unit of the old build; the B files are the units of the new build
that may now hold its functions.  Prints, per mangled symbol (kernels and the
out-of-line device functions they call), one of

    same        the text from the label to .Lfunc_end is identical
    differs     both sides have it, the text is not identical
    only in A   no B file has it
    only in B   a B file has it, A does not

and exits non-zero unless every line says `same`.  Block labels and function
ordinals (.LBB<n>_<k>, .Lfunc_end<n>, ...) count functions from the top of
their file, so <n> is taken out before comparing (in labels, in the "Header=BB<n>_<k>"
comments, and with it the column padding of a label line's comment); nothing
else is interpreted.
"""
import re
import sys

from isa_blocks import functions

ORDINAL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)\d+(_\d+)?\b")  # labels, and "Header=BB<n>_<k>" in comments


def table(path):
    # the comment after a label is padded to a column, so its blanks follow the ordinal's width
    return {name: [" ".join(ORDINAL.sub(r"\1\2", l).split()) if l.startswith(".L") else ORDINAL.sub(r"\1\2", l)
                   for l in lines] for name, lines in functions(path)}


def main():
    a = table(sys.argv[1])
    b = {}
    for p in sys.argv[2:]:
        for name, lines in table(p).items():
            if name in b and b[name] != lines:  # two new units disagree about one function
                a.setdefault(name, None)
                lines = None
            b[name] = lines
    verdicts = {}
    for name in sorted(set(a) | set(b)):
        if name not in b:
            v = "only in A"
        elif name not in a:
            v = "only in B"
        else:
            v = "same" if a[name] is not None and a[name] == b[name] else "differs"
        verdicts[v] = verdicts.get(v, 0) + 1
        print("%-10s %s" % (v, name))
    print("total: " + ", ".join("%d %s" % (n, v) for v, n in sorted(verdicts.items())))
    return 0 if set(verdicts) <= {"same"} else 1


if __name__ == "__main__":
    sys.exit(main())
