"""Compare the gfx950 instruction streams of the kernels of one source file between two trees.

Each tree's csrc/<FILE> is compiled to device assembly with the flags of parsenet_codebase_amd/build.py
(hipcc ... --cuda-device-only -S), the text is cut into one block per kernel symbol (from `<name>:` to its
`.Lfunc_end`), comments, directives and blank lines are dropped and local labels (.LBB<f>_<n>, whose function
number <f> moves when kernels are added to a file) are renumbered per kernel in order of first appearance.
A kernel template that gained a trailing integer parameter is paired with its instantiation at 0 in the new
tree (`...ELi0EEv` against `...EEv` in the mangled name: the earlier behaviour as the value 0).  Printed per
kernel of the OLD tree: identical / DIFFERS / missing in the new tree, and the kernels only the new tree has.
Exit status 1 if a kernel the two trees share differs.

Usage: python tools/kernel_asm_diff.py OLD_TREE NEW_TREE FILE.hip [FILE.hip ...]
   e.g. git archive HEAD~1 | tar -x -C _ab_prev; python tools/kernel_asm_diff.py _ab_prev . meanshift.hip meanshift_w.hip"""
import os
import re
import subprocess
import sys
import tempfile


def device_asm(tree, src):
    sys.path.insert(0, os.path.abspath(tree))
    try:
        for m in [m for m in sys.modules if m.startswith("parsenet_codebase_amd")]:
            del sys.modules[m]
        from parsenet_codebase_amd import build as B
        hipcc, flags = B.HIPCC, list(B.FLAGS)
    finally:
        sys.path.pop(0)
    path = os.path.join(tree, "parsenet_codebase_amd", "csrc", src)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True, text=True)
        with open(out) as fh:
            return fh.read()


def kernels(asm):
    """{symbol: [instruction lines]} with local labels renumbered per kernel."""
    out, name, lines, labels = {}, None, [], {}
    for raw in asm.splitlines():
        m = re.match(r"^(_Z\w+|pn_\w+):", raw)
        if m and name is None:
            name, lines, labels = m.group(1), [], {}
            continue
        if name is None:
            continue
        if raw.startswith(".Lfunc_end"):
            out[name], name = lines, None
            continue
        s = raw.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        s = re.sub(r"\.LBB\d+_\d+", lambda k: labels.setdefault(k.group(0), "L%d" % len(labels)), s)
        lines.append(re.sub(r"\s+", " ", s))
    return out


def main():
    old, new, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    for f in files:
        a, b = kernels(device_asm(old, f)), kernels(device_asm(new, f))
        print("%s: %d kernels in %s, %d in %s" % (f, len(a), old, len(b), new))
        for k in sorted(set(b) - set(a)):      # one more template parameter, at 0
            k0 = k.replace("Li0EEv", "Ev", 1)
            if k0 != k and k0 in a and k0 not in b:
                b[k0] = b.pop(k)
        for k in sorted(a):
            state = "missing" if k not in b else "identical" if a[k] == b[k] else "DIFFERS"
            bad += state == "DIFFERS"
            print("  %-9s %6d instructions  %s" % (state, len(a[k]), k[:150]))
        for k in sorted(set(b) - set(a)):
            print("  new       %6d instructions  %s" % (len(b[k]), k[:150]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
