"""CPU tests of the paired-end libraries (tests/pe_cases.py): the generator is deterministic, every library does on the CPU path what it
is meant to, and the oracle's SAM for it is the REFERENCE's (tests/golden/pelib_*, made by make_golden.py from oracle/_ref/bwaref) -- the
anchor of the oracle's paired-end stage records, which the reference itself cannot emit."""
import gzip
import os
import pytest
import common
import pe_cases as pc

G = common.GOLDEN


@pytest.fixture(scope="module")
def genome(small_index):
    return pc.load_genome(small_index["fa"])


def test_generator_is_deterministic(genome):
    a = pc.library(genome, "edges", 120)
    b = pc.library(genome, "edges", 120)
    assert a == b
    c = pc.make_library(genome, **{**{k: v for k, v in pc.LIBRARIES["edges"].items() if k in pc._GEN_KEYS}, "seed": 9, "n_pairs": 120})
    assert c[0] != a[0]
    assert {m[0] for m in a[2]} == {0, 1, 2, 3} and min(len(r) for r in a[0] + a[1]) >= 30
    r1, r2, meta = pc.library(genome, "ragged", 200)
    lens = [len(x) for x in r1 + r2]
    assert min(lens) >= 30 and max(lens) <= 301 and len(set(lens)) > 100      # (an insertion can add a base to a drawn length)


@pytest.mark.parametrize("name", list(pc.LIBRARIES))
def test_committed_reads_are_the_generators(genome, name):
    r1, r2, _ = pc.library(genome, name, pc.golden_pairs(name))
    for k, reads in ((1, r1), (2, r2)):
        want = gzip.open(os.path.join(G, f"pelib_{name}_{k}.fq.gz")).read()
        assert b"".join(b"@p%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)) == want


@pytest.mark.parametrize("name", list(pc.LIBRARIES))
def test_oracle_sam_equals_reference_sam(small_index, tmp_path, name):
    """Orientations other than FR, wide windows, ragged lengths and contig ends: oracle == reference, SAM byte for byte."""
    fqs = []
    for k in (1, 2):
        fqs.append(str(tmp_path / f"{name}_{k}.fq"))
        open(fqs[-1], "wb").write(gzip.open(os.path.join(G, f"pelib_{name}_{k}.fq.gz")).read())
    want = gzip.open(os.path.join(G, f"pelib_{name}.sam.gz")).read()
    assert pc.oracle_sam(small_index["prefix"], *fqs, flags=["-t", "4"]) == want


@pytest.mark.parametrize("name,flags", [(n, ()) for n in pc.LIBRARIES] + [("ragged", ("-A", "2"))])
def test_library_does_what_it_is_for(small_index, genome, tmp_path, name, flags):
    """The committed seeds: failed flags, window class, at least 30 rescued lists, the boundary lengths on rescued mates."""
    fq1, fq2, r1, r2, _ = pc.write_library(genome, name, tmp_path)
    ps, reads = pc.oracle_pe_stages(small_index["prefix"], fq1, fq2, str(tmp_path / "o.bin"), ["-t", "4", *flags])
    lens = [len(x) for p in zip(r1, r2) for x in p]
    pc.preconditions(name, ps, reads, lens)
    if name == "edges":                                        # anchors whose rescue window has its middle in the next contig
        assert pc.off_contig_windows(ps, reads, lens, [len(c) for c in genome]) >= 10
