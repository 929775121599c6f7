"""A PyTorch that is installed but fails to import must not take the library
with it.  sha1chunk.lib() imports torch first where it can,
only so that the process holds one HIP runtime; a torch that raises on import
-- ImportError, OSError for a shared object that cannot be opened,
RuntimeError -- is as good as none, and the host-only calls (binary2hex)
need no device at all.  Child processes: the import happens once per
process, and the broken torch must shadow the real one there only."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import importlib, sys
sys.path.insert(0, sys.argv[1])  # the repository
sys.path.insert(0, sys.argv[2])  # the directory with the torch that raises: found first
try:
    import torch
    raise SystemExit("the broken torch was not the one imported")
except SystemExit:
    raise
except BaseException as e:
    print("torch raises", type(e).__name__)
sys.modules.pop("torch", None)
pkg = importlib.import_module("congestion-control-with-bittorren_amd")
L = pkg.lib()
assert L is not None and L is pkg.lib()
assert pkg.binary2hex(b"\x00\xff") == "00ff"
print("library ok")
"""

RAISES = {
    "ImportError": 'raise ImportError("No module named torch._C")',
    "OSError": 'raise OSError("libamdhip64.so: cannot open shared object file")',
    "RuntimeError": 'raise RuntimeError("torch failed to initialise")',
}


@pytest.mark.parametrize("exc", sorted(RAISES))
def test_library_loads_when_torch_raises_on_import(tmp_path, exc):
    (tmp_path / "torch.py").write_text(RAISES[exc] + "\n")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path)], capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert f"torch raises {exc}" in r.stdout and "library ok" in r.stdout, r.stdout
