"""The shape matrix of the device prover's sweep (shard_shapes.py): the ledger of what it must cover, and the C
oracle pinned at those shapes: against oracle/pyref.py where Python is fast enough (P <= 64), and everywhere against
the oracle's own verifier, which evaluates the proof polynomial directly and shares no transform with the prover."""
import random

import pytest

import shard_shapes as SS
from janus_amd.vdaf import PRIO3_HISTOGRAM, PRIO3_SUM, PRIO3_SUMVEC
from oracle import oracle as O
from oracle import pyref

IDS = [SS.shape_id(v) for v in SS.INSTANCES]


def test_ledger():
    assert len(set(IDS)) == len(IDS)
    assert SS.unmet(SS.INSTANCES) == []
    for v in (SS.W2_P512, SS.W4_P256):
        assert v in SS.INSTANCES
    g = SS.geometry(SS.W2_P512)
    assert (g.P, g.W, g.chunk_mod_W) == (512, 2, 1) and g.chunk >= 3
    g = SS.geometry(SS.W4_P256)
    assert (g.P, g.W) == (256, 4) and 64 * g.P * g.W == SS.LDS_BYTES and g.chunk_mod_W != 0


def test_geometry_of_known_shapes():
    """The geometry function at shapes whose numbers DESIGN.md §5.6 states: the headline instance (P = 128, W = 4,
    32 KiB of LDS) and the cap (P = 1024, one wave holding 64 KiB)."""
    from janus_amd.vdaf import Prio3
    g = SS.geometry(Prio3.sum_vec(8, 1000, 88))
    assert (g.P, g.calls, g.W, g.chunk_mod_W, g.padded, g.streams) == (128, 91, 4, 0, 8, (8000, 176, 431))
    g = SS.geometry(Prio3.sum_vec(1, 600, 1))
    assert (g.P, g.calls, g.W, g.padded) == (1024, 600, 1, 0)
    g = SS.geometry(Prio3.sum(32))
    assert (g.two_wire, g.P, g.calls, g.W, g.streams) == (False, 64, 32, 1, (32, 1, 128))
    g = SS.geometry(Prio3.histogram(8, 1))  # 42 + 128 = 170 bytes: two message bytes in the last block
    assert (g.meas_mod_21, g.absorb_blocks, (42 + 16 * 8) % 168) == (8, 1, 2)
    g = SS.geometry(Prio3.histogram(18, 1))
    assert (g.meas_mod_21, (42 + 16 * 18) % 168) == (18, 162)


def _oracle(v):
    return O.Prio3Oracle(v.algo_id, v.bits, v.length, v.chunk_length, v.num_proofs)


def _measurements(v, rng):
    """The all-zero one, the all-max one (Histogram: the first and the last index) and a random one."""
    if v.algo_id == PRIO3_HISTOGRAM:
        return [0, v.length - 1, rng.randrange(v.length)]
    top = (1 << v.bits) - 1
    if v.algo_id == PRIO3_SUM:
        return [0, top, rng.randrange(top + 1)]
    return [[0] * v.length, [top] * v.length, [rng.randrange(top + 1) for _ in range(v.length)]]


def _pyref(v):
    if v.algo_id == PRIO3_SUM:
        return pyref.Prio3("sum", bits=v.bits)
    if v.algo_id == PRIO3_SUMVEC:
        return pyref.Prio3("sumvec", bits=v.bits, length=v.length, chunk=v.chunk_length)
    return pyref.Prio3("histogram", length=v.length, chunk=v.chunk_length)


@pytest.mark.parametrize("v", [v for v in SS.INSTANCES if v.P <= 64], ids=lambda v: SS.shape_id(v))
def test_c_shard_equals_pyref(v):
    rng = random.Random(v.meas_len * 131 + v.chunk_length)
    C, Py = _oracle(v), _pyref(v)
    assert C.sizes.client_rand == v.client_rand_len
    for m in _measurements(v, rng)[1:]:
        nonce, rand = rng.randbytes(16), rng.randbytes(v.client_rand_len)
        assert C.shard(m, nonce, rand) == Py.shard(m, nonce, rand)


@pytest.mark.parametrize("v", SS.INSTANCES, ids=IDS)
def test_c_shard_is_accepted_by_the_verifier(v):
    rng = random.Random(v.meas_len * 137 + v.chunk_length)
    C = _oracle(v)
    vk = rng.randbytes(16)
    for m in _measurements(v, rng):
        nonce, rand = rng.randbytes(16), rng.randbytes(v.client_rand_len)
        ps, lin, hin = C.shard(m, nonce, rand)
        rc, lshare, _, _ = C.prep_init(vk, 0, nonce, ps, lin)
        assert rc == 0
        assert C.helper_prep(vk, nonce, ps, hin, lshare)[0] == 0
