"""One ``unit sha256`` line per ``csrc/*.hip`` unit and one ``unit::symbol sha256`` line per function
symbol of its gfx950 device assembly: run on two trees and diff the output to show that a change kept
every kernel's machine code.  Each unit is compiled device-only to assembly (``--cuda-device-only -S``)
with the build's own flags (``build._flags`` and ``build._unit_flags`` of the tree that is digested);
the lines that contain ``__hip_cuid_`` (a per-invocation random symbol) are dropped and the rest is
hashed as text, whole and per ``.type NAME,@function`` .. ``.Lfunc_end`` range.  Nothing in the text is
interpreted.  CPU only; about a minute per unit.
python tools/isa_digest.py [--tree DIR] [--jobs N] [unit-substring ...]"""
import argparse, concurrent.futures as cf, hashlib, importlib.util, os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNC = re.compile(r"^\s*\.type\s+([^,\s]+),@function")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_isa_digest_build", os.path.join(tree, "ddim_cold_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, src, flags, tmp):
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    r = subprocess.run([build.HIPCC] + build._unit_flags(src, flags) + ["--cuda-device-only", "-S", src, "-o", out],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr[-4000:]}")
    with open(out) as fh:
        return [l for l in fh if "__hip_cuid_" not in l]


def sha(lines):
    return hashlib.sha256("".join(lines).encode()).hexdigest()[:32]


def symbols(lines):
    name, start = None, 0
    for i, l in enumerate(lines):
        m = FUNC.match(l)
        if m:
            name, start = m.group(1), i
        elif name is not None and l.startswith(".Lfunc_end"):
            yield name, lines[start:i + 1]
            name = None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="root of the checkout to digest (default: this one)")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("units", nargs="*")
    a = ap.parse_args(argv)
    build = load_build(os.path.abspath(a.tree))
    inc, _, abi = build._torch_paths()
    flags = build._flags(inc, abi)
    srcs = [s for s in build.sources() if s.endswith(".hip") and (not a.units or any(u in s for u in a.units))]
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max_workers=a.jobs) as ex:
        for src, lines in zip(srcs, ex.map(lambda s: assembly(build, s, flags, tmp), srcs)):
            unit = os.path.basename(src)
            print(f"{unit} {sha(lines)} ({len(lines)} lines)", flush=True)
            for name, body in sorted(symbols(lines)):
                print(f"{unit}::{name} {sha(body)}", flush=True)


if __name__ == "__main__":
    main()
