"""Hardware counters of the library's kernels: one `rocprofv3 --pmc <group>` pass per counter group and arm, each a run of its own
(no tracing flag beside --pmc), through the step runner of tools/steps.py: the first pass that ends abnormally is the last.

    python tools/pmc.py --kernels REGEX [--set tile|insts|icache|frame] [--out DIR] [--dry-run] [ARM ...] [-- probe argv]

ARM as in tools/ab.py (default: prod).  Prints count and mean per counter, per kernel as well for the sets icache and frame."""
import argparse
import collections
import csv
import re
import shutil
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from ab import PY, parse_arm  # noqa: E402
from steps import ROOT, Abnormal, run_step  # noqa: E402

STAGE3 = [PY, "tools/stage_probe.py", "--cfg", "3", "--frames", "4"]
# set -> counter groups (one pass each), whether the means are per kernel, default probe, time limit of a pass (s)
SETS = {
    "tile": (["SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_SMEM",
              "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS",
              "SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_SCA",
              "SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVES",
              "SQ_INST_CYCLES_VMEM SQ_WAIT_ANY SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR"], False, STAGE3, 200),
    "insts": (["SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_SMEM"], False, STAGE3, 200),
    "icache": (["SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE",
                "SQ_IFETCH SQ_IFETCH_LEVEL SQ_BUSY_CYCLES SQ_WAVE_CYCLES"], True, STAGE3, 200),
    "frame": (["SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES"], True,
              [PY, "bench.py", "--steps", "30", "--warmup", "5", "--no-cpu-baseline", "--no-extras"], 300),
}


def aggregate(csvs, per_kernel):
    """rocprofv3's *counter_collection.csv files -> {(kernel or '', counter): (count, mean)}, in the files' order."""
    acc = collections.defaultdict(list)
    for f in csvs:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                kernel = re.split(r"[(<]", re.sub(r"\(anonymous namespace\)::|^void ", "", r["Kernel_Name"]))[0] if per_kernel else ""
                acc[kernel, r["Counter_Name"]].append(float(r["Counter_Value"]))
    if not acc:
        raise ValueError("no counter rows")
    return {k: (len(v), sum(v) / len(v)) for k, v in acc.items()}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    probe = argv[argv.index("--") + 1:] if "--" in argv else None
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--kernels", required=True)
    ap.add_argument("--set", choices=SETS, default="tile")
    ap.add_argument("--out", default="build/pmc")
    ap.add_argument("--rocprof", default="rocprofv3")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("arms", nargs="*", metavar="ARM")
    a = ap.parse_args(argv[:argv.index("--")] if "--" in argv else argv)
    groups, per_kernel, default_probe, limit = SETS[a.set]
    probe = probe or default_probe
    out, lines = (ROOT / a.out).resolve(), []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say(f"tools/pmc.py --kernels '{a.kernels}' --set {a.set}: {len(groups)} pass(es) per arm of  rocprofv3 --pmc <group> "
        f"--kernel-include-regex '{a.kernels}' -- {' '.join(probe).replace(PY, 'python')}")
    try:
        for spec, env in [parse_arm(s) for s in a.arms or ["prod"]]:
            say(f"{spec}:")
            for i, grp in enumerate(groups, 1):
                d = out / f"{spec}_g{i}"
                cmd = [a.rocprof, "--pmc", *grp.split(), "--kernel-include-regex", a.kernels, "-d", str(d), "-o", "p",
                       "--output-format", "csv", "--", *probe]
                if a.dry_run:
                    print(f"  limit {limit} s, env {env}: {' '.join(cmd)}")
                    continue
                shutil.rmtree(d, ignore_errors=True)
                # TMPDIR: where rocprofv3 keeps its scratch files
                got = run_step(f"{spec}/g{i} ({grp})", cmd, {**env, "TMPDIR": "/tmp"}, limit, out / f"{spec}_g{i}.log",
                               lambda _: aggregate(sorted(d.rglob("*counter_collection.csv")), per_kernel))
                for (kernel, counter), (n, mean) in got.items():
                    say(f"{kernel:32s} " * per_kernel + f"{counter:28s} n={n:3d} mean={mean:.4g}")
    except Abnormal as e:
        say(str(e))
    if not a.dry_run:
        (out / "report.txt").write_text("\n".join(lines) + "\n")
    return 1 if lines[-1].startswith("STOPPED") else 0


if __name__ == "__main__":
    sys.exit(main())
