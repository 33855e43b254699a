"""What the test_host_*.py runners share: build the host mirror's C++ test programs (host/tests/*.cpp) and run one of them in a
mode.  `cpu` needs no GPU; `gpu` drives the device through the C ABI the way the Go shim would (no torch in that process)."""
import os
import subprocess

from gangfit import build


def _binary(path):
    build.build_native()
    build.build_host()
    assert os.path.exists(path), f"{os.path.basename(path)} was not built"
    return path


def _run(path, mode):
    p = subprocess.run([_binary(path), mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and " 0 failed" in p.stdout, p.stdout[-4000:]
    return p.stdout
