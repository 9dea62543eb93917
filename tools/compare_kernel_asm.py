"""Which kernels of one build's `make asm` output are instruction for instruction those of another's.
Usage: python tools/compare_kernel_asm.py PARENT.s NEW.s   (each sfm-python_amd/build/sfmba-gfx950.s of its tree)

A kernel's text runs from its label to its .Lfunc_end; the function's number inside block labels (.LBB<number>_<block>, and
the same in the loop comments) depends on how many kernels precede it in the file and is ignored, as is the padding
before a comment.  For a kernel that differs, the opcodes whose counts differ are listed as `opcode parent->new` (the
first word of every instruction line; labels, directives and comments are not counted): a kernel whose listed opcodes
are compares, selects, moves, waits and branches only does the same memory and floating-point work.
Exit status 1 when a kernel of the parent differs or is missing."""
import collections
import re
import sys


def kernels(path):
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, buf = m.group(1), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                out[name], name = buf, None
            else:
                buf.append(re.sub(r"\s+;", " ;", re.sub(r"BB\d+_", "BB_", line)))
    return out


def opcodes(lines):
    words = (ln.split(";")[0].split() for ln in lines)
    return collections.Counter(w[0] for w in words if w and not w[0].startswith(".") and not w[0].endswith(":"))


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    differ = [k for k in a if k not in b or a[k] != b[k]]
    print(f"{len(a)} kernels in the parent: {len(a) - len(differ)} unchanged instruction for instruction, {len(differ)} differ or are gone; "
          f"{len([k for k in b if k not in a])} new")
    for k in differ:
        print("  differs:", k)
        if k in b:
            ha, hb = opcodes(a[k]), opcodes(b[k])
            changed = [f"{op} {ha[op]}->{hb[op]}" for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op]]
            print(f"    {sum(ha.values())} -> {sum(hb.values())} instructions; opcode counts that differ:",
                  ", ".join(changed) if changed else "none (order or operands only)")
    for k in b:
        if k not in a:
            print("  new:", k)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
