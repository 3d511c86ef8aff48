"""Assembly gate of a refactor of the device code: every kernel of every .hip file of build.SOURCES against another checkout's, per
symbol, under a heading per file.

    python tools/isa_gate.py <the other checkout's root> [file.hip ...]     (files: only these, while iterating on one)

Both checkouts' files are compiled as tools/isa_audit.py compiles them.  'same': identical instruction for instruction (comments, directives and
block numbers stripped).  Otherwise: the instruction counts per loop and issue class (isa_audit.audit) and the resources (VGPRs, SGPRs,
spills, scratch, LDS, occupancy) of both, 'equal' when all of them agree.  CPU only: hipcc cross-compiles.
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path[:0] = [str(Path(__file__).resolve().parent.parent), str(Path(__file__).resolve().parent)]
from isa_audit import audit  # noqa: E402
from sim_a_splat_amd import build  # noqa: E402

KEYS = ("VGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize", "LDS Size", "Occupancy")


def kernels(root, src):
    tmp = Path(tempfile.mkdtemp(prefix="sas_gate_"))
    cmd = [build.hipcc_path(), build.OPT_LEVEL, "-std=c++17", f"--offload-arch={build.ARCH}", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", f"-I{root / 'include'}", "-c", "-x", "hip",
           str(root / "sim_a_splat_amd" / "csrc" / src), "-o", "t.o", "-save-temps"]
    err = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    for line in next(tmp.glob("*gfx950.s")).read_text().split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), {"lines": [], "res": {}})
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            cur["lines"].append(line)
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.get(m.group(1))
        m = re.search(r":\s{2,}([A-Za-z][\w ]*?)\s*(?:\[[\w/]+\])?: (\d+)", line)
        if m and cur is not None and m.group(1).strip() in KEYS:
            cur["res"][m.group(1).strip()] = int(m.group(2))
    for k in out.values():
        k["ins"] = [re.sub(r"BB\d+_", "BB_", s) for s in (l.split(";")[0].strip() for l in k["lines"]) if s and not s.startswith(".")]
        loops, per, _ = audit(k["lines"])
        k["loops"] = [(loops.get(name, 0), tuple(c.get(x, 0) for x in "VSWLGXR")) for name, c in per.items()]
    return out


def gate(other, src):
    a = kernels(other, src) if (other / "sim_a_splat_amd" / "csrc" / src).exists() else {}   # (a file the other checkout lacks: every kernel NEW)
    b = kernels(build.PKG.parent, src)
    print(f"==== {src}: {len(b)} kernels")
    for sym in sorted(set(a) | set(b)):
        name = subprocess.run(["c++filt", "-p", sym], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
        if sym not in a or sym not in b:
            k = a.get(sym) or b[sym]
            print(f"{'REMOVED' if sym in a else 'NEW':8s} {name}  {len(k['ins'])} instructions  {k['res']}")
            continue
        ka, kb = a[sym], b[sym]
        verdict = "same" if ka["ins"] == kb["ins"] else ("equal" if (ka["loops"], ka["res"]) == (kb["loops"], kb["res"]) else "DIFFER")
        print(f"{verdict:8s} {name}  {len(ka['ins'])} -> {len(kb['ins'])} instructions")
        if verdict == "DIFFER":
            for tag, k in (("other", ka), ("this", kb)):
                print(f"    {tag:5s} {k['res']}\n          loops (depth, V S W L G X R): {k['loops']}")


if __name__ == "__main__":
    for src in sys.argv[2:] or [p.name for p in build.SOURCES if p.suffix == ".hip"]:
        gate(Path(sys.argv[1]).resolve(), src)
