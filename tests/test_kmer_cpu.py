"""rsem-for-ebseq-calculate-clustering-info without a GPU: the Python restatement (tests/kmer_ref.py) against the files the
unmodified reference program wrote (tests/golden/clustering/), tests/kmer_check.cpp -- the arithmetic the device runs
(rsem_amd/csrc/kmer_block.hpp) and the program's FASTA reader, built with AddressSanitizer and UBSan -- and what the program does
before it needs a device: wrong argv, k = 0, an unreadable file.  Every comparison is equality."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kmer_ref as kr

from kmer_ref import GOLDEN, PROG, ROOT, recorded, recorded_id

CXX = shutil.which("g++")


def test_fixtures_are_there():
    names = {os.path.basename(c[2]) for c in recorded()}
    assert {"mixed.k25.ump", "mixed.k5.ump", "mixed.k28.ump", "mixed.k60.ump", "crlf.k25.ump", "tails.k27.ump", "tails.k55.ump"} <= names
    assert b"\r\n" in open(os.path.join(GOLDEN, "crlf.fa"), "rb").read()
    assert not open(os.path.join(GOLDEN, "tails.fa"), "rb").read().endswith(b"\n")


@pytest.mark.parametrize("case", recorded(), ids=recorded_id)
def test_restatement_equals_recorded(case):
    fa, k, u = case
    assert kr.ump(open(fa, "rb").read(), k) == open(u, "rb").read()


def test_restatement_reader_rules():
    names, seqs, dropped = kr.read_fasta(b">a b\tc\r\nacgu\r\nRN\r\n>e\n>f\n\n\n>g\nAC")
    assert names == [b"a b\tc\r", b"g"] and dropped == [b"e", b"f"]
    assert seqs[0].tolist() == [0, 1, 2, 4, 4, 4, 4, 4] and seqs[1].tolist() == [0, 1]
    assert kr.read_fasta(b"ACGT\n>x\nAC\n")[0] == []  # the first line is no header: no entry
    assert kr.shared_counts([np.array([0, 0, 0, 0], np.uint8), np.array([1, 0, 0], np.uint8)], 2) == ([3, 1], 2)
    assert kr.shared_counts([np.array([0, 1, 0, 1, 0], np.uint8), np.array([2, 2], np.uint8)], 2)[0] == [0, 0]  # repeated inside only


def test_batching_rule():
    seqs = [np.array([0] * 10 + [1] * 3, np.uint8), np.array([1] * 5, np.uint8)]
    assert kr.bucket_histogram(seqs, 1) == [(0, 10), (1, 8)]
    assert kr.expected_batches(seqs, 1, 100) == [18]
    assert kr.expected_batches(seqs, 1, 17) == [10, 8]
    assert kr.expected_batches(seqs, 1, 3) == [10, 8]  # each bucket above the budget: a batch of its own
    assert kr.expected_batches(seqs, 20, 3) == []


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if CXX is None:
        pytest.skip("needs g++")
    exe = os.path.join(str(tmp_path_factory.mktemp("kmer_check")), "kmer_check")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "kmer_check.cpp"), "-o", exe])
    return exe


def test_check_program_pipeline(checker):
    out = subprocess.run([checker, "pipeline"], check=True, capture_output=True, text=True).stdout
    assert re.fullmatch(r"ok \d+\n", out), out
    assert int(out.split()[1]) >= (18 + 5 + 8 + 1) * 2  # the random inputs, large k, the seams, one k-mer: whole and in batches at least


def test_check_program_limits(checker):
    """the constructions of tests/kmer_limits.py alone: large k, separators on the word, lane and tile seams, one k-mer"""
    out = subprocess.run([checker, "limits"], check=True, capture_output=True, text=True).stdout
    assert re.fullmatch(r"ok \d+\n", out) and int(out.split()[1]) >= (5 + 8 + 1) * 2, out


@pytest.mark.parametrize("name", ["mixed.fa", "crlf.fa", "tails.fa"])
def test_check_program_reader(checker, name):
    path = os.path.join(GOLDEN, name)
    names, seqs, dropped = kr.read_fasta(open(path, "rb").read())
    out = subprocess.run([checker, "fasta", path], check=True, capture_output=True).stdout
    want = kr.warnings_text(dropped)
    want += b"".join(n + b"\t" + bytes(b"ACGTN"[c] for c in s) + b"\n" for n, s in zip(names, seqs))
    assert out == want
    assert len(names) >= 4


def test_check_program_reader_corner_files(checker, tmp_path):
    for i, data in enumerate([b"", b"\n>x\nAC\n", b">only_header", b">a\n\r\n>b\nacg", b">a\nAC\n\n\nGT\n>b\n>c\nT\n"]):
        path = os.path.join(str(tmp_path), "c%d.fa" % i)
        open(path, "wb").write(data)
        names, seqs, dropped = kr.read_fasta(data)
        out = subprocess.run([checker, "fasta", path], check=True, capture_output=True).stdout
        want = kr.warnings_text(dropped)
        want += b"".join(n + b"\t" + bytes(b"ACGTN"[c] for c in s) + b"\n" for n, s in zip(names, seqs))
        assert out == want, data
    assert subprocess.run([checker, "fasta", os.path.join(str(tmp_path), "missing.fa")], capture_output=True).returncode == 2


@pytest.fixture(scope="module")
def program():
    from rsem_amd import build
    build.build()
    assert os.path.exists(PROG), "rsem-for-ebseq-calculate-clustering-info was not built"
    return PROG


@pytest.mark.parametrize("argv", [[], ["25"], ["25", "in.fa"], ["25", "in.fa", "out.ump", "--bogus"], ["25", "in.fa", "out.ump", "--device"]])
def test_program_wrong_argv(program, argv):
    r = subprocess.run([program] + argv, capture_output=True, text=True)
    assert r.returncode == 255
    assert r.stdout.startswith("Usage: rsem-for-ebseq-calculate-clustering-info k input_reference_fasta_file output_file")


@pytest.mark.parametrize("k", ["0", "-3", "abc"])
def test_program_refuses_k_below_1(program, tmp_path, k):
    out = os.path.join(str(tmp_path), "o.ump")
    r = subprocess.run([program, k, os.path.join(GOLDEN, "mixed.fa"), out], capture_output=True, text=True)
    assert r.returncode == 255 and "at least 1" in r.stderr
    assert not os.path.exists(out)


def test_program_unreadable_file(program, tmp_path):
    out = os.path.join(str(tmp_path), "o.ump")
    r = subprocess.run([program, "25", os.path.join(str(tmp_path), "missing.fa"), out], capture_output=True, text=True)
    assert r.returncode == 255 and "Cannot open" in r.stderr and "missing.fa" in r.stderr
    assert not os.path.exists(out)


def test_library_refuses_invalid_arguments_without_a_device():
    """the checks come before the device is touched: they answer on a machine that has none"""
    from rsem_amd import capi
    off = np.array([0, 4, 6], np.uint64)
    codes = np.array([0, 1, 2, 3, 4, 0], np.uint8)
    for bad_off, bad_codes, k in [(off, codes, 0), (np.array([0, 5, 3], np.uint64), codes, 2), (np.array([1, 4, 6], np.uint64), codes, 2),
                                  (off, np.array([0, 1, 2, 3, 5, 0], np.uint8), 2)]:
        with pytest.raises(capi.RsemHipError) as e:
            capi.kmer_shared_counts(bad_off, bad_codes, k)
        assert e.value.status == -1  # RSEM_ERR_INVALID
    shared, info = capi.kmer_shared_counts(off, codes, 7)  # no transcript is as long as k: all zeros, no device needed
    assert shared.tolist() == [0, 0] and info["n_kmers"] == 0 and info["n_batches"] == 0
