"""What a Device owns, on the CPU under AddressSanitizer + UBSan: tools/devmem_check.cpp
includes the runtime's own header (corda_amd/csrc/runtime.hpp) and links it against
counting fakes of hipMalloc / hipFree / hipHostMalloc / hipHostFree, the event calls,
hipStreamDestroy and hipSetDevice. It checks that the visit reaches every buffer, event
and stream the structs hold (against their sizeof), that the idle release leaves exactly
the kept buffers and the account equals their bytes, that ~Device -- of a full and of a
half-initialised Device -- leaves nothing live and the account at zero, and that two
Devices charge the accounts of their own ids."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
@pytest.mark.skipif(not os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_runtime.h")), reason="HIP headers absent")
def test_device_ownership_asan_ubsan(tmp_path):
    exe = str(tmp_path / "devmem_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", ROCM_INCLUDE, "-o", exe,
                           os.path.join(ROOT, "tools", "devmem_check.cpp"), "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["dev_bufs"] > 0 and st["pin_bufs"] > 0 and st["events"] > 0 and st["streams"] == 7, st
    # the idle release keeps the fixed tables, both ECDSA counters and the encoder's table
    assert st["kept_dev_bufs"] == 6, st
