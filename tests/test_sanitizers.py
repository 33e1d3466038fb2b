"""AddressSanitizer + UndefinedBehaviorSanitizer runs of the CPU-side code (VERDICT r1 weak item 12,
SURVEY §5): the oracle (oracle/sancheck.c) and the engine's host code — the layout builder and the host
instantiation of engine_math.h through the emulation (tests/host_emu/sancheck.cc, built host-only), and the
library's own host code behind the C-ABI, the handle's lifetimes above all (tests/host_emu/handlecheck.cc:
layout-only handles and the failure paths of creation, linked with the library's kernel objects) —
over every parity configuration. GPU sanitizers are not available on this pool; these are host-only."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.configs import config_descs, cost_descs, ext_cases
from tests.shape_sweep import make as sweep_make
from towr2025_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle", "build", "sancheck")
EMU = os.path.join(ROOT, "tests", "host_emu", "build", "sancheck")
HANDLES = os.path.join(ROOT, "tests", "host_emu", "build", "handlecheck")


def _cases():
    out = {k: (v, []) for k, v in config_descs().items()}
    out.update({k: (v, []) for k, v in cost_descs().items()})
    out.update(ext_cases())
    # shapes of the seeded sweep (tests/shape_sweep.py); 13, 85, 86 and 131 have a foot that never touches down
    out.update({f"sweep_seed_{s}": (sweep_make(s)[0].to_desc(), []) for s in (0, 10, 13, 35, 59, 85, 86, 131)})
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def binaries():
    for d, exes in ((os.path.join(ROOT, "oracle"), (ORACLE,)), (os.path.join(ROOT, "tests", "host_emu"), (EMU, HANDLES))):
        subprocess.check_call(["make", "-s", "-C", d, "sanitize"])
        assert all(os.path.exists(exe) for exe in exes)
    return ORACLE, EMU, HANDLES


def _write(path, desc, data):
    with open(path, "wb") as f:
        f.write(bytes(desc))
        f.write(struct.pack("<i", len(data)))
        for kind, index, arr in data:
            a = np.ascontiguousarray(arr, dtype=np.float64).ravel()
            f.write(struct.pack("<iiq", kind, index, a.size))
            f.write(a.tobytes())


@pytest.mark.parametrize("name", sorted(CASES))
def test_sanitized_host_code(binaries, tmp_path, name):
    desc, data = CASES[name]
    p = str(tmp_path / "problem.bin")
    _write(p, desc, data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for exe in binaries:
        r = subprocess.run([exe, p], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), f"{os.path.basename(exe)}: rc {r.returncode}\n{r.stderr[-3000:]}"
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
