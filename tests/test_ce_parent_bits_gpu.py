"""Every output bit of klab_ce_count, klab_ce_fwd, klab_ce_wsum, klab_ce_fwd_opts and klab_ce_fwd_distill (csrc/ce.hip) against
the digests recorded from the commit before the three cross-entropy files became one (tests/golden/ce_parent_bits.json, written by
tools/record_ce_bits.py; cases and digest: tests/ce_bits_cases.py).

rule                                                              -> shape
  the dispatch (one-pass NIT 8 | 16, two-pass; f32)                 -> bf16 V = 8, 2056, 16384 | 16392, 32768 | 32776, 40000; f32 V = 4, 1028, 4104
  the norm and reduce kernels stride 256 threads over the rows      -> rows = 6 and 261
  row strides ld, ldt > V                                           -> ld = V + 16, ldt = V + 24, sentinels behind every row of both"""
import json
import os

import pytest

from tests import ce_bits_cases as C

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ce_parent_bits.json")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_the_case_list_and_names_its_commit(recorded):
    assert len(recorded["parent"]) == 40 and int(recorded["parent"], 16) >= 0
    assert sorted(recorded["digests"]) == sorted(C.all_ids())
    assert all(len(d) == 64 for d in recorded["digests"].values())


@pytest.mark.gpu
@pytest.mark.parametrize("rows,V,dt", C.SHAPES)
def test_every_output_bit_is_the_parent_commits(recorded, rows, V, dt):
    from klab_multimodalmodel_amd import ops
    got = C.shape_digests(ops, rows, V, dt)
    bad = [cid for cid, d in got.items() if recorded["digests"][cid] != d]
    assert not bad, f"{len(bad)} of {len(got)} cases differ from commit {recorded['parent'][:12]}: {bad[:8]}"
