"""The coordinate order of the sorted BAM output, restated for the tests from the record's own bytes (SAM specification 4.2: refID at
bytes 4..8, pos at 8..12, flag at 18..20 of a record that starts with its block_size) and Python's stable sorted().  Nothing here calls
the library under test."""
import struct

import numpy as np

import bam_ref

HD = "@HD\tVN:1.6\tSO:coordinate\n"


def fields(rec):
    """(refID, pos, reverse) of one record."""
    ref_id, pos = struct.unpack_from("<ii", rec, 4)
    (flag,) = struct.unpack_from("<H", rec, 18)
    return ref_id, pos, flag >> 4 & 1


def order_key(rec):
    """refID as an unsigned number (-1 after every contig), pos (-1 first), forward before reverse; ties keep their input order."""
    ref_id, pos, rev = fields(rec)
    return ref_id & 0xffffffff, pos, rev


def stable_sort(records):
    return sorted(records, key=order_key)


def sorted_bytes(buf):
    """Concatenated records -> the same records concatenated in coordinate order."""
    return b"".join(stable_sort(bam_ref.split_records(buf)))


def packed_key(rec, n_seqs, longest):
    """The documented 64-bit key (include/bwahip.h) of a record, from the layout's description alone."""
    ref_id, pos, rev = fields(rec)
    pos_bits = (longest + 1).bit_length()
    return (n_seqs if ref_id < 0 else ref_id) << (pos_bits + 1) | (pos + 1) << 1 | rev


def make_runs(records, n_runs, rng, empty=None):
    """Cut `records` (input order) into n_runs consecutive pieces of uneven size (piece `empty` has no record) and sort every piece:
    a list of record lists."""
    cuts = sorted(rng.sample(range(1, len(records)), n_runs - 1)) if n_runs > 1 else []
    bounds = [0] + cuts + [len(records)]
    if empty is not None and n_runs > 1:
        e = min(max(empty, 1), n_runs - 1)                         # piece e = [bounds[e], bounds[e + 1]) loses its records to piece e - 1
        bounds[e] = bounds[e + 1]
    return [stable_sort(records[bounds[k]:bounds[k + 1]]) for k in range(n_runs)]


def run_arrays(run, key_of):
    off = np.zeros(len(run) + 1, dtype=np.int64)
    if run:
        off[1:] = np.cumsum([len(r) for r in run])
    return b"".join(run), np.array([key_of(r) for r in run], dtype=np.uint64), off
