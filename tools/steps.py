"""The step runner of tools/ab.py and tools/pmc.py: one GPU program at a time, and none after one that ended abnormally.

Every step is a fresh child under `timeout -k 10 <limit>`; stdout is captured (and kept beside the log), stderr goes to the log.
This module never imports torch or the library: the runner holds no GPU.  There are no retries."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
FAULT = "an illegal memory access was encountered"   # the HIP runtime's sentence: a fault even where the program goes on and exits 0


class Abnormal(Exception):
    """A step ended abnormally.  The caller starts nothing further, writes what it has with str(this), and exits with status 1."""


def run_step(name, argv, env_add, limit, log, extract):
    """Run argv from the repository root and return extract(stdout).  The caller's own SAS_* variables are not inherited: a step
    sees the knobs of env_add and no others.  Raises Abnormal on a non-zero exit status (124 / 137: the limit), on the fault
    sentence in stdout or the log, and on output that extract cannot read."""
    log = Path(log)
    log.parent.mkdir(parents=True, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAS_")}
    with open(log, "wb") as err:
        p = subprocess.run(["timeout", "-k", "10", str(limit), *argv], env={**env, **env_add}, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=err)
    out = p.stdout.decode(errors="replace")
    log.with_suffix(".out").write_text(out)
    status = f"exit status {p.returncode}"
    if p.returncode == 0:
        if FAULT in out or FAULT in log.read_text(errors="replace"):
            status += ", GPU fault reported"
        else:
            try:
                return extract(out)
            except Exception as e:   # whatever the extractor trips over: the output is not what the probe prints
                status += f", output not readable ({type(e).__name__}: {e})"
    raise Abnormal(f"STOPPED at step {name}: {status}; log {log}; nothing was started after it")
