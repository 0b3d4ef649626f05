"""The wrapper the GPU tests share for the stand-alone check programs under tools/ (one
.hip file with its own main that prints one PASS / FAIL line)."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def build_and_run(name, tmp_path, opt):
    """Compiles tools/<name>.hip for gfx950 at `opt` into tmp_path and runs it: exit status 0
    and a stdout that starts with PASS."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / name
    subprocess.run([hipcc, "--offload-arch=gfx950", opt, "-o", str(exe), str(ROOT / "tools" / f"{name}.hip")],
                   check=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.startswith("PASS"), p.stdout + p.stderr
