"""tools/steps.py, tools/ab.py and tools/pmc.py without a GPU: the order and isolation of the steps, that nothing is started after a
step that ended abnormally, the extractors on the probes' committed outputs, the reading against the one made by hand in
profiles/host_owners_ab.txt, and the counter aggregation.  The stand-in probes are plain Python that never imports torch."""
import collections
import csv
import json
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import ab  # noqa: E402
import pmc  # noqa: E402

PROFILES = ROOT / "profiles"
STAGE_LINE = ('{"cfg": 3, "n": 1000000, "wh": [1920, 1080], "stats": {"n_visible": 999442, "n_isect": 4718213}, "stage_ms": {"project": 0.0749, '
              '"scan": 0.005, "scatter": 0.0048, "sort": 0.0059, "blend": 0.1037, "tail": 0.0047, "total": 0.1984}}')
LOWER = {"project_ms": ab.LO, "tile_ms": ab.LO, "total_ms": ab.LO}


@pytest.fixture
def variants(tmp_path, monkeypatch):
    """The tool looks for variants/ under a scratch root holding lib_x.so; the caller's own knobs must not reach a step."""
    (tmp_path / "variants").mkdir()
    (tmp_path / "variants" / "lib_x.so").write_bytes(b"")
    monkeypatch.setattr(ab, "ROOT", tmp_path)
    monkeypatch.setenv("SAS_LIB_PATH", "/caller/lib.so")
    monkeypatch.setenv("SAS_CULL", "1")
    return tmp_path


def test_order_and_isolation(variants, monkeypatch, capsys):
    seen = []
    show = "import os, json; print(json.dumps({'pid': os.getpid(), 'env': {k: v for k, v in os.environ.items() if k.startswith('SAS_')}}))"
    monkeypatch.setitem(ab.PROBES, "show", ([sys.executable, "-c", show], 20,
                                            lambda out: seen.append(json.loads(out)) or {"pid": seen[-1]["pid"]}, {"pid": ab.LO}))
    assert ab.main(["--probes", "show", "--out", str(variants / "out"), "prod", "x,SAS_CULL=0"]) == 0
    lib = str(variants / "variants" / "lib_x.so")
    assert Path(lib).is_absolute()
    assert [s["env"] for s in seen] == [{}, {"SAS_LIB_PATH": lib, "SAS_CULL": "0"}] * 2
    assert len({s["pid"] for s in seen}) == 4
    labels = re.findall(r"^(\d\d_\S+)", capsys.readouterr().out, re.M)
    assert labels == ["01_prod", "02_x,SAS_CULL=0", "03_prod", "04_x,SAS_CULL=0"]
    # refused before any step starts
    for arms in (["prod", "x,HIP_FORCE_DEV_KERNARG=1"], ["prod", "x,SAS_LIB_PATH=/other.so"], ["prod,SAS_CULL", "x"], ["prod", "missing"]):
        with pytest.raises(SystemExit):
            ab.main(["--probes", "show", "--out", str(variants / "out"), *arms])
    assert len(seen) == 4


STAND_IN = """#!{exe}
import pathlib, sys, time
side, mode = sys.argv[-2:]
with open(side, "a") as f:
    f.write("started\\n")
if "-d" in sys.argv:   # in rocprofv3's place: the counter file of a pass
    d = pathlib.Path(sys.argv[sys.argv.index("-d") + 1])
    d.mkdir(parents=True)
    (d / "p_counter_collection.csv").write_text("Kernel_Name,Counter_Name,Counter_Value\\nk_tile_lazy<false>(int),SQ_WAVES,1\\n")
if len(open(side).readlines()) == 2:
    if mode == "sleep":
        time.sleep(30)
    elif mode == "fault":
        print("HIP error: an illegal memory access was encountered", file=sys.stderr)
    else:
        sys.exit(int(mode))
print('{line}')
"""
ENDS = {"1": "exit status 1;", "134": "exit status 134;", "139": "exit status 139;", "sleep": "exit status 124;",
        "fault": "exit status 0, GPU fault reported;"}


@pytest.mark.parametrize("tool", ["ab", "pmc"])
@pytest.mark.parametrize("mode", list(ENDS))
def test_nothing_starts_after_an_abnormal_step(tool, mode, variants, monkeypatch, capsys):
    """Step 2 of 4 ends abnormally: two programs were started, the partial report names the step, its status and its log, exit 1."""
    script, side, out = variants / "stand_in.py", variants / "side.txt", variants / "out"
    script.write_text(STAND_IN.format(exe=sys.executable, line=STAGE_LINE))
    script.chmod(0o755)
    if tool == "ab":
        monkeypatch.setitem(ab.PROBES, "stand", ([str(script), str(side), mode], 1, ab.stage_ms, LOWER))
        status, step = ab.main(["--probes", "stand", "--out", str(out), "prod", "x"]), "02_x/stand"
        log = out / "02_x_stand.log"
    else:
        monkeypatch.setitem(pmc.SETS, "icache", (["C1 C2", "C3"], True, None, 1))
        status = pmc.main(["--kernels", "k", "--set", "icache", "--out", str(out), "--rocprof", str(script), "prod", "x", "--", str(side), mode])
        step, log = "prod/g2 (C3)", out / "prod_g2.log"
    assert status == 1
    assert side.read_text() == "started\n" * 2
    report = (out / "report.txt").read_text()
    assert report == capsys.readouterr().out
    assert f"STOPPED at step {step}: {ENDS[mode]} log {log};" in report
    assert log.is_file() and ("illegal memory access" in log.read_text()) == (mode == "fault")


def test_extractors_read_the_committed_outputs():
    """Each file carries the stray libdrm line in front of the probe's text."""
    stray = "/opt/amdgpu/share/libdrm/amdgpu.ids: No such file or directory\n"
    extract = {k: v[2] for k, v in ab.PROBES.items()}
    for name, probe in (("r05_bench.json", "bench"), ("r05_bench_driver_cmd_1.json", "bench_driver")):
        text = (PROFILES / name).read_text()
        d = json.loads(text)
        got = extract[probe](stray + text)
        assert got == {"value": d["value"], "door_a_sync": d["door_a_sync"]["value"], "door_a_async": d["door_a_async"]["value"],
                       "cold_start": d["cold_start"]["value"]}
        assert set(ab.PROBES[probe][3]) <= set(got)
    text = (PROFILES / "r05_config_fps.txt").read_text()
    assert text.startswith(stray)
    assert extract["config_fps"](text) == {"cfg1": 38868, "cfg2": 19874, "cfg3": 6717, "cfg5": 2453}
    text = (PROFILES / "r05_env_steps.txt").read_text()
    assert text.startswith(stray)
    assert extract["demo_env"](text) == {"demo_steps": 7973}
    stages = {'project': 0.0306, 'scan': 0.0046, 'scatter': 0.0046, 'sort': 0.0052, 'blend': 0.043, 'tail': 0.0046, 'total': 0.0926}
    assert extract["door_b"](text) == {"door_b_steps": 8033, **{f"door_b_{k}_ms": v for k, v in stages.items()}}
    assert extract["vec_env"](text) == {"vec1": 9336, "vec4": 3947, "vec16": 1064}
    assert extract["stage3"](stray + "upload s 0.41\n" + STAGE_LINE + "\n") == {"project_ms": 0.0749, "tile_ms": 0.1037, "total_ms": 0.1984}
    assert extract["stage3_plain"]('upload s 0.4\n{"cfg": 3, "us_per_blocking_frame": 181.5}\n') == {"frame_us": 181.5}
    assert extract["py_overhead"](stray + "tensor.data_ptr()                            0.09\n"
                                  "Rasterizer.render, 50 Gaussians at 64x64, not blocking: 19.81 per call (Python + C ABI + three launches)\n"
                                  "the bare C-ABI call in the same loop:                    18.33 per call\n") \
        == {"render_us": 19.81, "bare_us": 18.33, "py_us": pytest.approx(1.48)}
    assert extract["host_overhead"](stray + "n=1000: host enqueue 23.2 us/frame, end-to-end 141.0 us/frame\n") \
        == {"enqueue_us": 23.2, "end_to_end_us": 141.0}
    # the calls that need no scene: every call median the probe prints, and nothing but what the row declares
    for probe, name, want in (("cloud", "point_cloud.txt", {"cloud1_512": 3.650, "cloud1_1024": 7.187, "cloud1_4096": 28.642, "cloud16_512": 3.879,
                                                            "cloud16_1024": 7.475, "cloud16_4096": 29.118}),
                              ("fuse", "tsdf_fuse.txt", {"fuse2_128": 0.078, "fuse2_256": 0.202, "fuse32_128": 0.319, "fuse32_256": 1.807}),
                              ("match", "match_points.txt", {"match113831": 0.764, "match292247": 1.871})):
        assert extract[probe](stray + (PROFILES / name).read_text()) == want
        assert set(ab.PROBES[probe][3]) == set(want) and not any(ab.PROBES[probe][3].values())   # (all lower-is-better)
    for probe in ("stage3", "bench", "config_fps", "door_b", "vec_env", "demo_env", "py_overhead", "host_overhead", "cloud", "fuse", "match"):
        with pytest.raises(Exception):   # a probe that died: the libdrm line and a traceback
            ab.declared(probe)(stray + "Traceback (most recent call last):\n")


def test_reading_equals_the_one_made_by_hand():
    """Call E of profiles/host_owners_ab.txt: the parent's ranges and every figure outside them on the slow side, as written there."""
    text = (PROFILES / "host_owners_ab.txt").read_text().split("Call E")[1].split("Call D")[0]
    lines = text.splitlines()
    cols = lines[1].split()[1:]
    rows = [(ln.split()[0], ln.split()[0][3:], dict(zip(cols, map(float, ln.split()[1:])))) for ln in lines[2:12]]
    assert [r[0] for r in rows] == ["01_parent", "02_new", "03_parent", "04_new", "05_parent", "06_new", "07_parent", "08_new", "09_parent", "10_new"]
    higher = {m: not m.endswith("_us") for m in cols}
    ranges, outside = ab.read_rows(rows, "parent", higher)
    by_hand = {m: (float(a), float(b)) for m, a, b in re.findall(r"(\w+) (-?[\d.]+) \.\. (-?[\d.]+)[,.]", "\n".join(lines[12:14]))}
    assert len(by_hand) == 8 and {m: ranges[m] for m in by_hand} == by_hand
    got = {m: [(label[:2], round(pct, 1)) for label, _, pct in out] for m, out in outside.items() if m in by_hand}
    assert got == {"value": [], "door_a_sync": [("04", 2.2)], "cold_start": [("02", 0.2), ("04", 0.3), ("10", 0.1)],
                   "py_us": [("04", 54.8)], "enqueue_us": [], "vec1": [("04", 13.7), ("10", 0.5)], "vec4": [],
                   "vec16": [("04", 0.4), ("10", 0.0)]}
    assert rows[1][2]["value"] == ranges["value"][0]   # 02_new equals the parent's lowest: inside
    report = ab.report(["header"], rows, "parent", higher)
    assert "    door_a_sync  04_new 5225.3 (2.2 % under)\n" in report
    assert "    vec1         04_new 16243.0 (13.7 % under), 10_new 18719.0 (0.5 % under)\n" in report
    assert "    py_us        04_new 9.72 (54.8 % over)\n" in report
    assert "value, " in report.splitlines()[-1] and report.endswith("all inside.\n")


def test_counter_aggregation():
    path = PROFILES / "r05_pmc_fetch_size.csv"
    direct = collections.defaultdict(list)
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").removeprefix("void ").split("(")[0].split("<")[0]
            direct[name, r["Counter_Name"]].append(float(r["Counter_Value"]))
    got = pmc.aggregate([path], per_kernel=True)
    assert {"k_project", "k_tile_lazy", "k_relayout"} <= {k for k, _ in got} and {c for _, c in got} == {"FETCH_SIZE"}
    assert got == {k: (len(v), pytest.approx(sum(v) / len(v), rel=1e-12)) for k, v in direct.items()}
    every = [v for vs in direct.values() for v in vs]
    assert pmc.aggregate([path], per_kernel=False) == {("", "FETCH_SIZE"): (len(every), pytest.approx(sum(every) / len(every), rel=1e-12))}
    with pytest.raises(ValueError):
        pmc.aggregate([], per_kernel=False)
