"""Are the kernels of one source file the same device code on two commits?  Compares, kernel by kernel, the instruction
streams of two assembly listings of the same .hip file:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S csrc/optim.hip -o new.s      # in this tree
    hipcc ... -S csrc/optim.hip -o old.s                                                        # in a checkout of the other commit
    python tools/isa_compare.py old.s new.s

Kernels are matched by demangled name.  A kernel that gained a defaulted trailing template argument (the table / argument
block types SpanTab, GsqArgs, DwArgs of the *_lrmul_f32 work) is matched with its old name; the instantiations on the new
types (SpanTabLM, GsqArgsLM, DwArgsLM) exist on one side only and are listed as such.  Comments, directives and the
numbering of local labels are ignored; everything else must be equal, line for line.  Exit status 1 if any matched kernel
differs or a kernel of the first listing has no partner."""
import re
import subprocess
import sys

DEFAULTED = ("SpanTab", "GsqArgs", "DwArgs")


def kernels(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):\s*; @", ln)
        if m:
            cur = out[m.group(1)] = []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        t = ln.split(";")[0].strip()
        if t and not t.startswith("."):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, r))


def key(name):
    s = name.replace("(anonymous namespace)::", "").split("(")[0]
    for t in DEFAULTED:
        s = s.replace(f", {t}>", ">").replace(f"<{t}>", "")
    return re.sub(r"^void", "", re.sub(r"\s+", "", s))      # (a template's demangled name carries its return type)


def main(old, new):
    a, b = kernels(old), kernels(new)
    da, db = demangle(list(a)), demangle(list(b))
    partner = {key(v): k for k, v in db.items()}
    bad = 0
    for k, v in da.items():
        kb = partner.pop(key(v), None)
        if kb is None:
            print(f"MISSING  {v}")
            bad += 1
        elif a[k] != b[kb]:
            print(f"DIFFERS  {len(a[k]):6d} / {len(b[kb]):6d} instructions  {key(v)}")
            bad += 1
        else:
            print(f"same     {len(a[k]):6d} instructions  {key(v)}")
    for kb in partner.values():
        print(f"new      {len(b[kb]):6d} instructions  {db[kb].replace('(anonymous namespace)::', '').split('(')[0]}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
