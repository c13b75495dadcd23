"""CPU-only: every stand-alone tool under tools/ compiles for gfx950 from the committed files alone (nothing is run).

The tracked files (`git ls-files`) are copied to a temporary directory first, so a header the tools need but git ignores
fails here instead of on the next person's checkout."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import REPO

HIPCC = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17"]
# the flags of a tool's own build line (its header), and the stamped builds tools/refresh_profiles.sh runs; default: one plain build
BUILDS = {"clock_probe.hip": [["-DW24_TIMING", "-L/opt/rocm/lib", "-lrocm_smi64", "-lpthread"]],
          "wino24_ubench.hip": [[], ["-DW24_TIMING"]],
          "wgrad_ubench.hip": [[], ["-DWGW_TIMING"]]}


def _tracked_files():
    try:
        r = subprocess.run(["git", "-c", f"safe.directory={REPO}", "ls-files", "-z"], cwd=REPO, capture_output=True, timeout=60)
    except (OSError, subprocess.TimeoutExpired):
        return None
    return [f for f in r.stdout.decode().split("\0") if f] if r.returncode == 0 else None


def test_every_tool_builds_from_the_tracked_files(tmp_path):
    files = _tracked_files()
    if not files:
        pytest.skip("not a git checkout")
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    src = tmp_path / "src"
    for f in files:
        if os.path.isfile(os.path.join(REPO, f)):
            (src / f).parent.mkdir(parents=True, exist_ok=True)
            shutil.copy2(os.path.join(REPO, f), src / f)
    tools = sorted(f for f in files if os.path.dirname(f) == "tools" and f.endswith(".hip"))
    assert tools
    jobs = [(t, i, extra) for t in tools for i, extra in enumerate(BUILDS.get(os.path.basename(t), [[]]))]

    def build(job):
        tool, i, extra = job
        out = tmp_path / f"{os.path.basename(tool)[:-4]}_{i}"
        r = subprocess.run([HIPCC, *FLAGS, str(src / tool), "-o", str(out), *extra], cwd=src, capture_output=True, text=True,
                           timeout=600)
        return tool, extra, r.returncode, r.stderr

    with ThreadPoolExecutor(max_workers=4) as pool:
        results = list(pool.map(build, jobs))
    failed = [f"{tool} {' '.join(extra)}: exit {rc}\n{err[-1500:]}" for tool, extra, rc, err in results if rc != 0]
    assert not failed, "\n".join(failed)
