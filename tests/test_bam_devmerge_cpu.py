"""What the device merge has that needs no device: the ctypes mirrors of its two structs against the C compiler's view of
include/bwahip.h, and the HBM formula the stream driver's budget is counted with, on cases computed by hand."""
import ctypes as C
import os
import subprocess

import common
from common import bw


def test_struct_mirrors_match_the_header(built, tmp_path):
    fields = {"bwahip_devmerge_stats_t": bw.DevMergeStats, "bwahip_sort_dev_t": bw.SortDevStats}
    src = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "bwahip.h"', "int main(void) {"]
    for name, cls in fields.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in cls._fields_:
            lines.append(f'    printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(common.ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, text=True).stdout.splitlines())
    for name, cls in fields.items():
        assert int(got[name]) == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, f"{name}.{f}"
    # every member of the C structs is mirrored: the sizes leave no room for another one
    assert C.sizeof(bw.DevMergeStats) == 7 * 8 + 4 * 8 and bw.SortDevStats.dev.offset + C.sizeof(bw.DevMergeStats) == C.sizeof(bw.SortDevStats)


def test_hbm_formula_on_hand_computed_cases(built):
    """need = runs + work + work / 8 with runs = raw + 16 n + 8 r, work = 48 n + min(blocks(raw), piece_blocks) x 326 730 + 64 MiB, where
    326 730 = 4 x 65 280 (two inputs, two outputs) + 2 x 31 + 65 536 (slot) + 12 (member length and offset)."""
    need = bw.bam_devmerge_hbm_need
    assert need(0, 0, 0, 1) == 67108864 + 8388608
    assert need(65280, 100, 1, 1024) == 66888 + 67440394 + 8430049
    assert need(65281, 100, 1, 1024) == 66889 + (67440394 + 326730) + (67440394 + 326730) // 8          # one byte more: a second block
    assert need(10 ** 9, 3 * 10 ** 6, 10, 256) == 1048000080 + 294751744 + 36843968
    assert need(10 ** 9, 3 * 10 ** 6, 10, 4096) - need(10 ** 9, 3 * 10 ** 6, 10, 256) == (4096 - 256) * 326730 * 9 // 8
    for bad in ((-1, 0, 0, 1), (0, -1, 0, 1), (0, 0, -1, 1), (0, 0, 0, 0), (0, 0, 0, 4097)):
        assert need(*bad) == -1, bad
    # what the driver's decision relies on: more bytes, records or runs never need less
    a = need(5 * 10 ** 6, 15000, 3, 1024)
    assert a < need(5 * 10 ** 6 + 1, 15000, 3, 1024) and a < need(5 * 10 ** 6, 15001, 3, 1024) and a < need(5 * 10 ** 6, 15000, 4, 1024)
