"""The private counting of the recalibration-table stage without a device.  tests/recal_slots_check.cpp plays one workgroup of
csrc/k_recal.hip serially through the helpers both compile (csrc/recal_tables.h: the claim of a slot, the LDS cell indices, the flush) under
the address and undefined-behaviour sanitizers, as a child process; bwahip_recal_hbm_need is checked against the sizes it is made of."""
import os
import shutil
import subprocess

import pytest

import common
from common import bw

CSRC = os.path.join(common.ROOT, "bwa-mem-gpu_amd", "csrc")


def test_slots_claim_count_and_flush_under_asan_ubsan(tmp_path):
    """Shares with no record that takes part (every slot unclaimed at the flush), one quality, as many qualities as slots, more (the
    overflow path), quality bytes above 93, cycles 255 and 256 on both mates; the index helpers at max_cycle 1 and 65 536.  The dense
    table of every share equals rc_walk's word for word, and nothing is read or written outside an array of the LDS arrays' sizes."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "recal_slots_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + CSRC, os.path.join(common.ROOT, "tests", "recal_slots_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr[-3000:]


def test_recal_hbm_need(built):
    def want(sum_len, max_cycle, with_mask):
        work = 16 * 94 * (1 + 2 * (max_cycle or 1024) + 17) + ((sum_len + 7) // 8 if with_mask else 0) + 4096
        return work + work // 8

    for sum_len in (0, 1, 7, 8, 9, 1000003, 3100000000, 2 ** 40 - 1):
        for max_cycle in (0, 1, 151, 700, 1024, 65536):
            for with_mask in (False, True):
                assert bw.recal_hbm_need(sum_len, max_cycle, with_mask) == want(sum_len, max_cycle, with_mask), (sum_len, max_cycle, with_mask)
    assert bw.recal_hbm_need(0, 0, False) == bw.recal_hbm_need(0, 1024, False) == (16 * 94 * 2066 + 4096) * 9 // 8
    assert bw.recal_hbm_need(3100000000, 0, True) - bw.recal_hbm_need(3100000000, 0, False) in (387500000 * 9 // 8, 387500000 * 9 // 8 + 1)
    for bad in ((-1, 0, False), (2 ** 40, 0, False), (100, -1, True), (100, 65537, False)):
        assert bw.recal_hbm_need(*bad) == -1, bad
