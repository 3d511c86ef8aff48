"""A/B of library variants and SAS_* knobs, alternating inside ONE GPU call, stopping at the first step that ends abnormally:

    python tools/ab.py [--rounds N] [--probes a,b,...] [--out DIR] [--dry-run] ARM ARM ...
    ARM := name[,SAS_X=value...]      name: prod (the in-tree library) or variants/lib_<name>.so

The first arm is the reference; a round runs the arms in the order given and --rounds (default 2) repeats the list.  The report
lists every run, the reference's range per metric inside this call, and every figure of the other arms outside that range on the
slow side.  That spread is the project's margin: no threshold is made up here, and the exit status is 0 when every step ran."""
import argparse
import ast
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from steps import ROOT, Abnormal, run_step  # noqa: E402

# Settings::from_env of sas_api.cpp, and the projection launcher's SAS_PROJ_MIX.  SAS_LIB_PATH comes from the arm's name.
KNOBS = {"SAS_SLOTS", "SAS_PAIR", "SAS_GROUP", "SAS_QUAD", "SAS_DIRECT", "SAS_CULL", "SAS_SEG_FACTOR", "SAS_DIRECT_BUDGET_MB",
         "SAS_QUAD_TILES", "SAS_RING_RESTART", "SAS_PROJ_MIX"}
PY = sys.executable
HI, LO = True, False   # per metric: larger is better / smaller is better


def last_json(out):
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def stage_ms(out):
    s = last_json(out)["stage_ms"]
    return {"project_ms": s["project"], "tile_ms": s["blend"], "total_ms": s["total"]}


def bench(out):
    d = last_json(out)
    return {k: d[k] if k == "value" else d[k]["value"] for k in ("value", "door_a_sync", "door_a_async", "cold_start") if k in d}


def prose(pattern, read):
    """Extractor of a probe that prints prose: ONE anchored expression; read() turns its matches into the metrics."""
    return lambda out: read(re.findall(pattern, out, re.M))


def door_b(m):
    (steps, stages), = m
    return {"door_b_steps": float(steps), **{f"door_b_{k}_ms": v for k, v in ast.literal_eval(stages).items()}}


def sectioned(name):
    """read() of a probe that prints a heading per configuration and a line per size under it.  Its expression matches either, as
    (the heading's number, '', '') or ('', size, ms): {name.format(heading's number, size): ms} in the order printed."""
    def read(m):
        got, head = {}, None
        for h, size, ms in m:
            if h:
                head = h
            else:
                got[name.format(head, size)] = float(ms)
        return got
    return read


def rows(names):
    """read() of a probe that prints, per scene, one line per call with its device time first: the expression matches
    (the call's words, ms); names maps those words to a metric's stem, and the scenes are numbered in the order printed."""
    def read(m):
        got = {}
        for words, ms in m:
            k = 1 + sum(1 for g in got if g.rsplit("_", 1)[0] == names[words])
            got[f"{names[words]}_{k}"] = float(ms)
        return got
    return read


def stage(cfg):
    return ([PY, "tools/stage_probe.py", "--cfg", str(cfg)], 200, stage_ms, {"project_ms": LO, "tile_ms": LO, "total_ms": LO})


# name -> argv, time limit (s), extractor (stdout -> {metric: float}), {metric: larger is better}.  200 / 300 s as the shell scripts
# had them; chosen here where they had none: stage1, stage2 and stage3_plain 200 like stage3, bench_driver 300 like bench,
# config_fps / door_b / vec_env / demo_env as tools/refresh_profiles.sh limits them, py_overhead and host_overhead 200, cloud / fuse /
# match 300 like bench (their torch baselines run once: --torch-repeats 1).
PROBES = {
    "stage1": stage(1), "stage2": stage(2), "stage3": stage(3), "stage5": stage(5),
    "stage3_plain": ([PY, "tools/stage_probe.py", "--cfg", "3", "--frames", "300", "--plain"], 200,
                     lambda out: {"frame_us": last_json(out)["us_per_blocking_frame"]}, {"frame_us": LO}),
    "bench": ([PY, "bench.py", "--steps", "300", "--no-cpu-baseline"], 300, bench,
              {"value": HI, "door_a_sync": HI, "door_a_async": HI, "cold_start": HI}),
    "bench_driver": ([PY, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-extras"], 300,
                     bench, {"value": HI, "cold_start": HI}),
    "config_fps": ([PY, "tools/config_fps.py", "1", "2", "3"], 300,
                   prose(r"^cfg(\d+): .* -> (\d+) frames/s", lambda m: {f"cfg{c}": float(v) for c, v in m}),
                   {"cfg1": HI, "cfg2": HI, "cfg3": HI}),
    "door_b": ([PY, "tools/door_b_breakdown.py"], 200,
               prose(r"^\{.*\} us per step; total [\d.]+ us -> (\d+) env steps/s\n(?:.*\n)*?isolated frame stage ms: (\{.*\})$", door_b),
               {"door_b_steps": HI, "door_b_project_ms": LO, "door_b_blend_ms": LO, "door_b_total_ms": LO}),
    "vec_env": ([PY, "tools/vec_env_probe.py", "1", "4", "16"], 300,
                prose(r"^(\d+) envs x .*?per-env poses: (\d+) steps/s", lambda m: {f"vec{e}": float(v) for e, v in m}),
                {"vec1": HI, "vec4": HI, "vec16": HI}),
    "demo_env": ([PY, "examples/demo_synthetic_env.py"], 200,
                 prose(r"^(\d+) env steps/s, ", lambda m: {"demo_steps": float(m[0])}), {"demo_steps": HI}),
    "py_overhead": ([PY, "tools/py_overhead_probe.py"], 200,
                    prose(r"^Rasterizer\.render, .*: ([\d.]+) per call .*\n(?:.*\n)*?the bare C-ABI call in the same loop: +([\d.]+) per call",
                          lambda m: {"render_us": float(m[0][0]), "bare_us": float(m[0][1]), "py_us": float(m[0][0]) - float(m[0][1])}),
                    {"render_us": LO, "bare_us": LO, "py_us": LO}),
    "host_overhead": ([PY, "tools/host_overhead.py"], 200,
                      prose(r"^n=\d+: host enqueue ([\d.]+) us/frame, end-to-end ([\d.]+) us/frame",
                            lambda m: {"enqueue_us": float(m[0][0]), "end_to_end_us": float(m[0][1])}),
                      {"enqueue_us": LO, "end_to_end_us": LO}),
    # the calls that need no scene: the medians of the blocking calls (ms); the probes exit 1 when their torch baselines disagree
    "cloud": ([PY, "tools/cloud_probe.py", "--torch-repeats", "1"], 300,
              prose(r"^(?:E = (\d+) \(|  K = (\d+): sample call ([\d.]+) ms)", sectioned("cloud{}_{}")),
              {f"cloud{e}_{k}": LO for e in (1, 16) for k in (512, 1024, 4096)}),
    "fuse": ([PY, "tools/fuse_probe.py", "--torch-repeats", "1"], 300,
             prose(r"^(?:C = (\d+) views:|  (\d+)\^3 voxels: fuse call ([\d.]+) ms)", sectioned("fuse{}_{}")),
             {f"fuse{c}_{n}": LO for c in (2, 32) for n in (128, 256)}),
    "match": ([PY, "tools/match_probe.py"], 300,
              prose(r"^\d+ x (\d+) = \S+ pairs: +([\d.]+) ms per call", lambda m: {f"match{t}": float(ms) for t, ms in m}),
              {"match113831": LO, "match292247": LO}),
    # the list readers behind a full-sort frame, per scene (1: the Gym cameras, 2: the 1920x1080 view of config 3): ms per view of the tile
    # stage (k_blend + the reader) for the lift probes, of the call's device events for the backward probe
    "lift": ([PY, "tools/lift_probe.py"], 300,
             prose(r"^lift_labels \((votes \+ seen|seen only)\) +([\d.]+) \[", rows({"votes + seen": "lift", "seen only": "lift_seen"})),
             {f"{k}_{s}": LO for k in ("lift", "lift_seen") for s in (1, 2)}),
    "lift_features": ([PY, "tools/lift_features_probe.py"], 300,
                      prose(r"^lift_features (C=\d+ \((?:sums \+ weight|weight only)\)) +([\d.]+) \[",
                            rows({f"C={c} ({w})": f"liftf{c}{s}" for c in (3, 8, 32, 256) for w, s in (("sums + weight", ""), ("weight only", "w"))})),
                      {f"liftf{c}{s}_{k}": LO for c in (3, 8, 32, 256) for s in ("", "w") for k in (1, 2)}),
    "grad": ([PY, "tools/grad_probe.py"], 300,
             prose(r"^render_backward (screen_space \(k_grad_tiles\)|\(k_grad_tiles \+ k_grad_project\)) +([\d.]+) \[",
                   rows({"screen_space (k_grad_tiles)": "grad_tiles", "(k_grad_tiles + k_grad_project)": "grad_full"})),
             {f"{k}_{s}": LO for k in ("grad_tiles", "grad_full") for s in (1, 2)}),
}


def declared(probe):
    """The probe's extractor held to the metrics its row declares: one that is missing makes the output unreadable."""
    _, _, extract, metrics = PROBES[probe]

    def read(out):
        got = extract(out)
        return {m: float(got[m]) for m in metrics}
    return read


def parse_arm(spec):
    """'name[,SAS_X=value...]' -> (spec, environment additions); refuses what is not a knob and a variant that is not there."""
    name, *sets = spec.split(",")
    env = dict(s.split("=", 1) for s in sets if "=" in s)
    bad = [s for s in sets if s.split("=", 1)[0] not in KNOBS or "=" not in s]
    if bad:
        raise SystemExit(f"arm {spec!r}: {bad} not accepted; an arm sets only {sorted(KNOBS)}")
    if name != "prod":
        lib = ROOT / "variants" / f"lib_{name}.so"
        if not lib.is_file():
            raise SystemExit(f"arm {spec!r}: {lib} does not exist")
        env["SAS_LIB_PATH"] = str(lib)
    return spec, env


def read_rows(rows, ref, higher):
    """rows: [(label, arm, {metric: value})].  -> ({metric: (lowest, highest) of arm ref}, {metric: [(label, value, per cent beyond
    the range's slow end)]} of the other arms' figures outside it on the slow side; a figure equal to the end is inside)."""
    ranges, outside = {}, {}
    for m, hi in higher.items():
        mine = [v[m] for _, arm, v in rows if arm == ref and m in v]
        if not mine:
            continue
        lo_end, hi_end = ranges[m] = (min(mine), max(mine))
        end = lo_end if hi else hi_end
        outside[m] = [(label, v[m], abs(v[m] - end) / abs(end) * 100 if end else float("nan")) for label, arm, v in rows
                      if arm != ref and m in v and (v[m] < end if hi else v[m] > end)]
    return ranges, outside


def num(v):
    return f"{v:.4g}" if abs(v) < 100 else f"{v:.1f}"


def report(header, rows, ref, higher):
    ranges, outside = read_rows(rows, ref, higher)
    w = max([9] + [len(label) for label, _, _ in rows])
    lines = list(header) + ["", f"{'run':{w}s} " + " ".join(f"{m:>11s}" for m in higher)]
    lines += [f"{label:{w}s} " + " ".join(f"{num(v[m]) if m in v else '-':>11s}" for m in higher) for label, _, v in rows]
    lines += [f"  {ref}'s ranges: " + ", ".join(f"{m} {num(a)} .. {num(b)}" for m, (a, b) in ranges.items()), "  Outside on the slow side:"]
    for m, out in outside.items():
        word = "under" if higher[m] else "over"
        lines += [f"    {m:12s} " + ", ".join(f"{label} {num(v)} ({pct:.1f} % {word})" for label, v, pct in out)] if out else []
    inside = [m for m, out in outside.items() if not out]
    return "\n".join(lines + ([f"  {', '.join(inside)}: all inside."] if inside else [])) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--probes", default="stage3,bench")
    ap.add_argument("--out", default="build/ab")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("arms", nargs="+", metavar="ARM")
    a = ap.parse_args(argv)
    arms = [parse_arm(s) for s in a.arms]
    probes = {p: PROBES[p] for p in a.probes.split(",")}
    # a metric two of the chosen probes share (value of bench and bench_driver) carries its probe's name
    names = [m for _, _, _, ms in probes.values() for m in ms]
    col = {(p, m): m if names.count(m) == 1 else f"{p}.{m}" for p, (_, _, _, ms) in probes.items() for m in ms}
    higher = {col[p, m]: hi for p, (_, _, _, ms) in probes.items() for m, hi in ms.items()}
    out = (ROOT / a.out).resolve()
    header = [f"tools/ab.py: arms {' | '.join(a.arms)} (reference: {a.arms[0]}), {a.rounds} round(s), alternating inside one call."]
    header += [f"  {p:13s} {' '.join(cmd).replace(PY, 'python')}   (limit {limit} s)" for p, (cmd, limit, _, _) in probes.items()]
    rows, stopped = [], ""
    try:
        for i in range(a.rounds * len(arms)):
            spec, env = arms[i % len(arms)]
            label = f"{i + 1:02d}_{spec}"
            rows.append((label, spec, {}))
            for p, (cmd, limit, _, _) in probes.items():
                if a.dry_run:
                    print(f"{label}/{p}: env {env} limit {limit} s: timeout -k 10 {limit} {' '.join(cmd)}")
                    continue
                got = run_step(f"{label}/{p}", cmd, env, limit, out / f"{label}_{p}.log", declared(p))
                rows[-1][2].update({col[p, m]: v for m, v in got.items()})
    except Abnormal as e:
        stopped = f"\n{e}\n"
    if a.dry_run:
        return 0
    text = report(header, rows, a.arms[0], higher) + stopped
    (out / "report.txt").write_text(text)
    print(text, end="")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
