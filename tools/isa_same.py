"""Are the kernels of two trees the same machine code?  No GPU needed:
    python tools/isa_same.py PARENT NEW [--map REGEX=REPL ...] [--files a.hip,b.hip] > profiles/tuner_fmt_isa_same.txt
PARENT and NEW are each a checkout (compiled here to gfx950 assembly with ITS OWN build.FLAGS / FILE_FLAGS, as tools/isa_hist.py
does) or a directory of *.s files made that way.  Every kernel of PARENT is paired with the kernel of NEW that has the same demangled
name (template arguments included, parameter list dropped) after the renames of RENAMES and --map, the instruction streams are
normalised -- symbol names of kernels and of their LDS arrays, .LBB<n>_ labels, `;` comments -- and compared line by line.  Prints
SAME or the first differing line per kernel; exit status 1 on any difference and on any kernel left unpaired on either side."""
import argparse, concurrent.futures as cf, importlib.util, os, re, subprocess, sys, tempfile

# the translation units that include decimate_tile.hpp or tuner_mix.hpp (those a tree does not have are skipped)
FILES = ["kernels_tuner.hip", "kernels_tuner_bank.hip", "kernels_tuner_i16.hip", "kernels_small.hip", "kernels_fast.hip",
         "kernels_fast_filter.hip", "kernels_fast_orders.hip", "kernels_systolic.hip"]
# parent name -> new name: the int16 copies became the format argument 2 (IN_I16), `bool U8` the formats 1 (IN_U8) and 0 (IN_CF32)
A4 = r"(\d+, \d+, \d+, \d+), "
RENAMES = [(r"\bk_tuner_bank_c4_i16<" + A4, r"k_tuner_bank_c4<\1, 2, "),
           (r"\b(k_tuner_bank_c4|k_tuner_c4)<" + A4 + "true, ", r"\1<\2, 1, "),
           (r"\b(k_tuner_bank_c4|k_tuner_c4)<" + A4 + "false, ", r"\1<\2, 0, "),
           (r"\b(k_tuner_bank_crossfix|k_tuner_bank_cross|k_tuner_mix)_i16$", r"\1<2>"),
           (r"\b(k_tuner_bank_crossfix|k_tuner_bank_cross|k_tuner_crossfix|k_tuner_mix)<true>$", r"\1<1>"),
           (r"\b(k_tuner_bank_crossfix|k_tuner_bank_cross|k_tuner_crossfix|k_tuner_mix)<false>$", r"\1<0>")]


def assembly(tree, files, td):
    """{file: lines} of a checkout (compiled) or of a directory of .s files"""
    bpy = os.path.join(tree, "sdr_amd", "build.py")
    if not os.path.exists(bpy):
        return {f: open(os.path.join(tree, f)).read().splitlines() for f in sorted(os.listdir(tree)) if f.endswith(".s")}
    spec = importlib.util.spec_from_file_location("build_of_" + os.path.basename(td), bpy)
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    os.makedirs(td)

    def one(f):
        out = os.path.join(td, f + ".s")
        cmd = [B.HIPCC] + B.FLAGS + B.FILE_FLAGS.get(f, []) + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(B.CSRC, f), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True)
        return f, open(out).read().splitlines()
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        return dict(ex.map(one, [f for f in files if os.path.exists(os.path.join(B.CSRC, f))]))


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short(dem):
    """`void ns::k<1, true>(void const*, ns::S)` -> `ns::k<1, true>`: the parameter list is the last top-level (...)"""
    dem = dem.strip()
    if dem.endswith(")"):
        depth = 0
        for i in range(len(dem) - 1, -1, -1):
            depth += dem[i] == ")"
            depth -= dem[i] == "("
            if depth == 0:
                dem = dem[:i]
                break
    return re.sub(r"^void ", "", dem)


def kernels(asm):
    """{short demangled name: normalised instruction stream} of every kernel of every file"""
    found = {}
    for f, lines in asm.items():
        syms = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
        dem = demangle(syms)
        # every symbol of the file that an instruction may name: the kernels and the LDS arrays (.amdgpu_lds / .globl)
        known = set(syms) | {l.split()[1].rstrip(",") for l in lines if l.strip().startswith((".amdgpu_lds ", ".globl "))}
        sub = re.compile("|".join(sorted(map(re.escape, known), key=len, reverse=True)))
        for s in syms:
            start = next(i for i, l in enumerate(lines) if l.startswith(s + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".section"))
            body = []
            for l in lines[start + 1:end]:
                l = l.split(";")[0].strip()
                if l:
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", sub.sub("SYM", l)))
            name = short(dem[s])
            if name in found:
                raise SystemExit(f"two kernels named {name}")
            found[name] = body
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL", help="a rename of parent kernels, after the built-in table")
    ap.add_argument("--files", default=",".join(FILES))
    a = ap.parse_args()
    renames = RENAMES + [tuple(m.split("=", 1)) for m in a.map]
    with tempfile.TemporaryDirectory() as td:
        old = kernels(assembly(a.parent, a.files.split(","), os.path.join(td, "parent")))
        new = kernels(assembly(a.new, a.files.split(","), os.path.join(td, "new")))
    bad = 0
    taken = set()
    for name in sorted(old):
        to = name
        for rx, repl in renames:
            to = re.sub(rx, repl, to)
        arrow = name if to == name else f"{name} -> {to}"
        if to not in new or to in taken:
            print(f"UNPAIRED (parent)  {arrow}")
            bad += 1
            continue
        taken.add(to)
        x, y = old[name], new[to]
        d = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), None if len(x) == len(y) else min(len(x), len(y)))
        if d is None:
            print(f"SAME  {len(x):5d} lines  {arrow}")
        else:
            print(f"DIFF  line {d} of {len(x)} / {len(y)}  {arrow}\n    parent: {x[d] if d < len(x) else '<end>'}\n    new:    {y[d] if d < len(y) else '<end>'}")
            bad += 1
    for name in sorted(set(new) - taken):
        print(f"UNPAIRED (new)     {name}")
        bad += 1
    print(f"{len(old)} kernels of the parent, {len(new)} of the new tree, {bad} differing or unpaired")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
