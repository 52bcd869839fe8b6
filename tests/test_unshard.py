"""Prio3.unshard (host) against sums of the oracle's aggregate shares, for Count, Sum, SumVec and Histogram."""
import numpy as np
import pytest

from janus_amd.vdaf import Prio3
from oracle import oracle as O

CASES = {"count": Prio3.count(), "sum7": Prio3.sum(7), "sumvec_3_6_4": Prio3.sum_vec(3, 6, 4),
         "histogram_5_2": Prio3.histogram(5, 2)}


def _measurements(v, rng, n):
    if v.algo_id == O.COUNT:
        return rng.integers(0, 2, size=(n, 1), dtype=np.uint64)
    if v.algo_id == O.HISTOGRAM:
        return rng.integers(0, v.length, size=(n, 1), dtype=np.uint64)
    return rng.integers(0, 1 << v.bits, size=(n, v.length if v.algo_id == O.SUMVEC else 1), dtype=np.uint64)


@pytest.mark.parametrize("name", list(CASES))
def test_unshard_of_oracle_aggregate_shares(name):
    v = CASES[name]
    orc = O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length)
    assert orc.sizes.client_rand == v.client_rand_len
    vk, n = bytes(range(50, 66)), 9
    rng = np.random.default_rng(sum(map(ord, name)))
    meas = _measurements(v, rng, n)
    outs = ([], [])
    for i in range(n):
        nonce, rand = rng.bytes(16), rng.bytes(v.client_rand_len)
        ps, lis, his = orc.shard(meas[i], nonce, rand)
        for agg_id, share in ((0, lis), (1, his)):
            rc, _, out, _ = orc.prep_init(vk, agg_id, nonce, ps, share)
            assert rc == 0
            outs[agg_id].append(out)
    shares = [orc.aggregate(o) for o in outs]
    got = v.unshard(shares, n)
    if v.algo_id == O.HISTOGRAM:
        assert got == [int(np.sum(meas[:, 0] == b)) for b in range(v.length)]
    elif v.algo_id == O.SUMVEC:
        assert got == [int(meas[:, j].sum()) for j in range(v.length)]
    else:
        assert got == int(meas[:, 0].sum())
    # one share alone decodes to itself; the sum is mod p
    p = 2**64 - 2**32 + 1 if v.field_bytes == 8 else 2**128 - 28 * 2**64 + 1
    fb = v.field_bytes
    minus_one = (p - 1).to_bytes(fb, "little") * v.output_len
    one = (1).to_bytes(fb, "little") * v.output_len
    wrapped = v.unshard([minus_one, one, one], 1)
    assert wrapped == (1 if v.output_len == 1 and v.algo_id in (O.COUNT, O.SUM) else [1] * v.output_len)


def test_unshard_refuses_bad_input():
    v = Prio3.sum(8)
    with pytest.raises(ValueError):
        v.unshard([bytes(15)], 1)
    with pytest.raises(ValueError):
        v.unshard([b"\xff" * 16], 1)  # >= p
    with pytest.raises(ValueError):
        v.unshard([], 0)
    with pytest.raises(ValueError):
        Prio3.fixedpoint_boundedl2_vec_sum(16, 4).unshard([bytes(64)], 1)
