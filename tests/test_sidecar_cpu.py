"""What the host parts of the files beside a sorted BAM file share (bwa-mem-gpu_amd/csrc/sidecar_host.h), through a stand-alone program
(tests/sidecar_check.cpp) built with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import shutil
import subprocess

import common

INC = os.path.join(common.ROOT, "include")
CSRC = os.path.join(common.ROOT, "bwa-mem-gpu_amd", "csrc")


def test_sidecar_helpers_hold_under_the_sanitizers(tmp_path):
    """put32 / put64 bytes; write_all through short writes and EINTR, to no descriptor, to a closed one; check_refs at 2^31 - 1 / 2^31 and at a
    sum of 2^40 - 1 / 2^40 with and without the cap; the builder skeleton's latch: records before the refused one are counted, every later
    call returns the same code, a second finish is BWAHIP_EINVAL.  The header alone, with plain g++ and no HIP."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "sidecar_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I" + INC, "-I" + CSRC,
                           os.path.join(common.ROOT, "tests", "sidecar_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
