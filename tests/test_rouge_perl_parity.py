"""Parity: our ROUGE port vs the reference's ROUGE.pl.

The perl script's printed averages for the inputs below are stored, with
the inputs themselves, in tests/golden/rouge_perl_parity.json, so the
check needs neither perl nor a checkout of the reference."""

import json
import os

import numpy
import pytest

from nats_amd.decode.rouge import format_report

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "rouge_perl_parity.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {c["seed"]: c for c in json.load(f)["cases"]}


def _mk_files(tmp_path, seed=0, n=25):
    rng = numpy.random.RandomState(seed)
    vocab = ["w%d" % i for i in range(30)]
    ref = tmp_path / "ref.txt"
    sys_ = tmp_path / "sys.txt"
    with open(ref, "w") as fr, open(sys_, "w") as fs:
        for _ in range(n):
            fr.write(" ".join(rng.choice(vocab, size=rng.randint(1, 15))) +
                     "\n")
            fs.write(" ".join(rng.choice(vocab, size=rng.randint(0, 15))) +
                     "\n")
    return str(ref), str(sys_)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("nsize,metric", [(1, "N"), (2, "N"), (3, "N"),
                                          (1, "L")])
def test_matches_perl(tmp_path, golden, seed, nsize, metric):
    ref, sys_ = _mk_files(tmp_path, seed)
    case = golden[seed]
    # the stored perl output belongs to exactly these inputs
    with open(ref) as f:
        assert f.read() == case["ref"]
    with open(sys_) as f:
        assert f.read() == case["sys"]
    ours = format_report(ref, sys_, nsize, metric)
    # compare the three printed averages
    perl_nums = case["perl_last_line"]["%d-%s" % (nsize, metric)].split()
    our_nums = ours.strip().splitlines()[-1].split()
    assert len(perl_nums) == 3
    assert perl_nums == our_nums, (perl_nums, ours)
