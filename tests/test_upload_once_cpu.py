"""The upload-once type of the host code (bwa-mem-gpu_amd/csrc/upload_once.h), without a device: tests/upload_once_check.cpp instantiates
it on own.h's buffer over a fake of malloc / free and a counting fake upload, and is built with the address and undefined-behaviour
sanitizers and run as a child process -- no upload before set, one upload per set however many begins, a failed upload repeated by the
next begin, set with null clearing the host copy, and nothing alive at exit (which the sanitizer's leak check confirms)."""
import os
import shutil
import subprocess

import common

INC = os.path.join(common.ROOT, "include")
CSRC = os.path.join(common.ROOT, "bwa-mem-gpu_amd", "csrc")


def test_upload_once_holds_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "upload_once_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + INC, "-I" + CSRC,
                           os.path.join(common.ROOT, "tests", "upload_once_check.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
