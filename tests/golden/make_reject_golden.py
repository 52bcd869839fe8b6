"""Generate the reject_*.json fixtures: reports whose XOF streams hold a real rejected Field64 sample.

A raw sample >= p64 is a 2^-32 event per element, so the keys and nonces below were found by a
compiled brute-force search (tests/csrc/reject_search.c) and are recorded here as constants: a plain
run rebuilds the files in seconds, byte for byte. Nothing the searcher says is trusted: every hit is
re-derived with the C oracle's XOFs and with pyref before a file is written, every stream of every
report is scanned so that the rejected samples are exactly the listed ones, and the C oracle and pyref
must agree on every rejecting report.

    python tests/golden/make_reject_golden.py            # regenerate from the recorded hits
    python tests/golden/make_reject_golden.py --search   # redo the hunt (minutes to an hour of CPU)
                                                         # and print a new FOUND table to paste in
    python tests/golden/make_reject_golden.py --search mp_query mp_joint    # redo only these steps

Documents have make_golden.py's format plus a top-level "rejections" list of
{report, stream: meas|proofs|joint_rand|query_rand, raw_index, class}. inputs() gives the measurements,
nonces and client randomness again, so a test can shard the same reports for the leader role. Rejecting reports are honest
and untampered (verdict 0) and sit at lanes 0 and 63 of the first 64-report block and inside the
partial second block, between honest and tampered neighbours.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from oracle import pyref as R  # noqa: E402

P64 = 2**64 - 2**32 + 1
VK16 = bytes(range(16))
VK32 = bytes(range(32))
N = 70
LOG2_BUDGET = 36  # give up on a class only after 2^36 raw samples per wanted hit

# class -> (counter, raw index): the 8-byte little-endian counter that the searcher put in front of the
# class's TAIL to form the seed, blind or nonce
FOUND = {
    "count_meas": (2186837912, 0),
    "count_proofs_4": (691981587, 4),
    "count_proofs_early": (4346283772, 2),
    "count_query": (1575304869, 0),
    "mp_meas_odd": (99100663, 1),
    "mp_meas_last": (117068847, 31),
    "mp_meas_partial": (178302859, 10),
    "mp_meas_even": (570166311, 18),
    "mp_proofs": (93026119, 8),
    "mp_query": (2387613635, 0),
    "mp_joint": (3504044068, 0),
}

# what follows the counter in the searched value (seeds are 16 bytes for TurboSHAKE128, 32 for HMAC/AES)
TAIL = {
    "count_meas": b"cntmeas0", "count_proofs_4": b"cntprf00", "count_proofs_early": b"cntprf00",
    "count_query": b"cntqry00",
    "mp_meas_last": b"m" * 24, "mp_meas_partial": b"m" * 24, "mp_meas_even": b"m" * 24, "mp_meas_odd": b"m" * 24,
    "mp_proofs": b"p" * 24, "mp_query": b"mpqnonce", "mp_joint": bytes(24),
}
# fixture A: everything that does not fix the shape by its index
MPA = dict(bits=1, length=32, chunk=5, proofs=2)
# (the joint-randomness hit was searched with every other seeded value of its report fixed: the generator's
# seed comes from this name, so renaming the fixture means searching that hit again)
MPA_NAME = "reject_mp2_1x32_5"


def found_value(cls):
    return FOUND[cls][0].to_bytes(8, "little") + TAIL[cls]


def fixtures():
    """name -> (config, {lane: (class, stream)}); the shape of the partial-chunk fixture follows from the raw
    index that was found."""
    last, part = FOUND.get("mp_meas_last", (0, MPA["length"] - 1))[1], FOUND.get("mp_meas_partial", (0, 2))[1]
    # raw index meas_len - 1 with meas_len % 8 == 0: the replacement lies in a 64-byte keystream chunk that a
    # pass over exactly meas_len samples never generates
    assert last == MPA["length"] - 1 and MPA["length"] % 8 == 0 and part % 8 <= 5
    return {
        "reject_count": (dict(algo=O.COUNT, bits=0, length=0, chunk=0, proofs=1),
                         {0: ("count_meas", "meas"), 63: ("count_proofs_4", "proofs"),
                          65: ("count_proofs_early", "proofs"), 68: ("count_query", "query_rand")}),
        MPA_NAME: (dict(algo=O.SUMVEC_F64_MULTIPROOF, **MPA),
                   {0: ("mp_meas_even", "meas"), 31: ("mp_meas_odd", "meas"), 63: ("mp_meas_last", "meas"),
                    64: ("mp_proofs", "proofs"), 66: ("mp_query", "query_rand"), 69: ("mp_joint", "joint_rand")}),
        # a hit inside the last, partial 8-sample chunk of a share with meas_len % 8 != 0
        "reject_mp2_partial_chunk": (dict(algo=O.SUMVEC_F64_MULTIPROOF, bits=1, length=part + 2, chunk=2, proofs=2),
                                     {67: ("mp_meas_partial", "meas")}),
    }


# --------------------------------------------------------------------------- reference views of a report


def pyref_of(cfg):
    a = cfg["algo"]
    if a == O.COUNT:
        return R.Prio3("count")
    assert a == O.SUMVEC_F64_MULTIPROOF
    return R.Prio3("sumvec_f64_multiproof", proofs=cfg["proofs"], bits=cfg["bits"], length=cfg["length"],
                   chunk=cfg["chunk"])


def cfg_of_doc(doc):
    v = doc["vdaf"]
    return dict(algo=v["algo_id"], bits=v["bits"], length=v["length"], chunk=v["chunk_length"],
                proofs=v["num_proofs"])


def stream_inputs(P, vk, nonce, public_share, helper_input_share, joint_seed=None):
    """The helper's four sampled streams of one report: name -> (seed, dst, binder, elements wanted).
    The joint-randomness seed is the one the helper derives (its own part, the leader's from the public
    share), which is the prepare message of an honest report: joint_seed, or pyref's derivation."""
    S, V = P.S, P.valid
    out = {
        "meas": (helper_input_share[:S], P.dst("meas_share"), bytes([1]), V.MEAS_LEN),
        "proofs": (helper_input_share[S:2 * S], P.dst("proof_share"), bytes([P.PROOFS, 1]), V.PROOF_LEN * P.PROOFS),
        "query_rand": (vk, P.dst("query_randomness"), bytes([P.PROOFS]) + nonce, V.QUERY_RAND_LEN * P.PROOFS),
    }
    if V.JOINT_RAND_LEN:
        seed = joint_seed
        if seed is None:
            hmeas = P.helper_meas_share(1, helper_input_share[:S])
            part = P.joint_rand_part(1, helper_input_share[2 * S:3 * S], hmeas, nonce)
            seed = P.joint_rand_seed([public_share[:S], part])
        out["joint_rand"] = (seed, P.dst("joint_randomness"), bytes([P.PROOFS]), V.JOINT_RAND_LEN * P.PROOFS)
    return out


def rejected_raw_indices(raw: bytes, want: int):
    """Raw indices of the samples >= p64 met while taking `want` elements from the byte stream."""
    rej, taken, i = [], 0, 0
    while taken < want:
        x = int.from_bytes(raw[8 * i:8 * i + 8], "little")
        assert 8 * i + 8 <= len(raw), "stream too short for this many rejections"
        if x >= P64:
            rej.append(i)
        else:
            taken += 1
        i += 1
    return rej


def oracle_stream(P, seed, dst, binder, nbytes):
    if P.Xof is R.XofHmacSha256Aes128:
        return O.xof_hmac_aes(seed, dst, binder, nbytes)
    return O.xof_expand(seed, dst, binder, nbytes)


def report_rejections(P, vk, rep, use_pyref=False):
    """[(stream, raw_index)] of one fixture report, from the C oracle alone (or from pyref alone). The
    oracle's joint-randomness seed is the one its prep_init corrects to, which for a report that finishes
    must be the recorded prepare message."""
    nonce, ps = bytes.fromhex(rep["nonce"]), bytes.fromhex(rep["public_share"])
    his = bytes.fromhex(rep["helper_input_share"])
    joint_seed = None
    if P.valid.JOINT_RAND_LEN and not use_pyref:
        V = P.valid
        orc = O.Prio3Oracle(O.SUMVEC_F64_MULTIPROOF, V.bits, V.length, V.chunk, P.PROOFS)
        rc, _, _, joint_seed = orc.prep_init(vk, 1, nonce, ps, his)
        assert rc == 0 and (rep["verdict"] != 0 or joint_seed.hex() == rep["prep_msg"])
    out = []
    for name, (seed, dst, binder, want) in stream_inputs(P, vk, nonce, ps, his, joint_seed).items():
        nbytes = 8 * (want + 8)
        raw = P.Xof(seed, dst, binder).next(nbytes) if use_pyref else oracle_stream(P, seed, dst, binder, nbytes)
        out += [(name, i) for i in rejected_raw_indices(raw, want)]
    return sorted(out)


# --------------------------------------------------------------------------- building a fixture


def tamper(lps, sizes, keep_honest):
    """make_golden.tamper's kinds, leaving the rejecting reports alone."""
    kinds = []
    for i in range(lps.shape[0]):
        k = i % 6
        if i in keep_honest:
            kinds.append("")
        elif k == 1:
            lps[i, 1 + sizes.field_bytes] ^= 0x01
            kinds.append("verifier_bitflip")
        elif k == 3:
            lps[i, 0:sizes.field_bytes] = 0xFF
            kinds.append("verifier_ge_p")
        elif k == 5 and sizes.joint_rand_len:
            lps[i, -1] ^= 0x80
            kinds.append("joint_rand_part")
        else:
            kinds.append("")
    return kinds


def inputs(name, cfg, lanes, skip=()):
    """Seeded measurements, nonces and client randomness with the found values put in place."""
    rng = np.random.default_rng(sum(map(ord, name)) * 7919)
    orc = O.Prio3Oracle(cfg["algo"], cfg["bits"], cfg["length"], cfg["chunk"], cfg["proofs"])
    s = orc.sizes
    if cfg["algo"] == O.COUNT:
        meas = rng.integers(0, 2, size=(N, 1), dtype=np.uint64)
    else:
        meas = rng.integers(0, 1 << cfg["bits"], size=(N, cfg["length"]), dtype=np.uint64)
    nonces = rng.integers(0, 256, size=(N, 16), dtype=np.uint8)
    rands = rng.integers(0, 256, size=(N, s.client_rand), dtype=np.uint8)
    S = s.seed
    for lane, (cls, stream) in lanes.items():
        if cls in skip or cls not in FOUND:
            continue
        val = np.frombuffer(found_value(cls), np.uint8)
        if stream == "query_rand":
            nonces[lane] = val
        else:  # rand = k_helper_meas || k_helper_proofs || k_prove || blind_leader || blind_helper
            k = {"meas": 0, "proofs": 1, "joint_rand": 3}[stream]
            rands[lane, k * S:(k + 1) * S] = val
    return orc, meas, nonces, rands


def make(name, cfg, lanes):
    orc, meas, nonces, rands = inputs(name, cfg, lanes)
    s = orc.sizes
    vk = VK32 if s.verify_key == 32 else VK16
    ps, his, lps, _ = orc.client_leader_batch(vk, meas, nonces, rands, nthreads=8)
    kinds = tamper(lps, s, set(lanes))
    res = orc.helper_prep_batch(vk, nonces, ps, his, lps, nthreads=8, want_out_shares=True)
    reports = []
    for i in range(N):
        v = int(res["verdicts"][i])
        out = res["out_shares"][i].tobytes() if v == 0 else b""
        rep = {
            "measurement": [int(x) for x in meas[i]],
            "nonce": nonces[i].tobytes().hex(),
            "public_share": ps[i].tobytes().hex(),
            "helper_input_share": his[i].tobytes().hex(),
            "leader_prep_share": lps[i].tobytes().hex(),
            "tamper": kinds[i],
            "verdict": v,
            "prep_msg": res["prep_msgs"][i].tobytes().hex() if v == 0 else "",
            "out_share_sha256": hashlib.sha256(out).hexdigest() if v == 0 else "",
        }
        if i in lanes:
            rep["out_share"] = out.hex()
        reports.append(rep)
    rejections = [{"report": lane, "stream": stream, "raw_index": FOUND[cls][1], "class": cls}
                  for lane, (cls, stream) in sorted(lanes.items())]
    doc = {
        "generator": "tests/golden/make_reject_golden.py (C oracle oracle/prio3_oracle.c)",
        "parity": "pins GPU == C oracle == pyref on streams with a rejected sample; parity with prio 0.16.1 unpinned",
        "vdaf": {"algo_id": cfg["algo"], "bits": cfg["bits"], "length": cfg["length"],
                 "chunk_length": cfg["chunk"], "num_proofs": cfg["proofs"]},
        "verify_key": vk.hex(),
        "rejections": rejections,
        "reports": reports,
        "aggregate_share": res["agg"].hex(),
        "report_count": res["count"],
        "checksum": res["checksum"].hex(),
    }
    verify(doc)
    path = os.path.join(HERE, f"{name}.json")
    # one line per report and per top-level key
    doc["reports"] = "@REPORTS@"
    text = json.dumps(doc, indent=1).replace(
        '"@REPORTS@"', "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in reports) + "\n ]")
    doc["reports"] = reports
    with open(path, "w") as f:
        f.write(text)
    print(f"{name}: {N} reports, {len(rejections)} rejecting "
          f"({', '.join(r['class'] + '@' + str(r['raw_index']) for r in rejections)}), "
          f"{sum(r['verdict'] != 0 for r in reports)} refused -> {path}")


def verify(doc):
    """Every hit re-derived by the oracle and by pyref; no other rejection anywhere; both references
    agree on every rejecting report, which finishes."""
    cfg = cfg_of_doc(doc)
    P, vk = pyref_of(cfg), bytes.fromhex(doc["verify_key"])
    orc = O.Prio3Oracle(cfg["algo"], cfg["bits"], cfg["length"], cfg["chunk"], cfg["proofs"])
    listed = sorted((r["report"], r["stream"], r["raw_index"]) for r in doc["rejections"])
    for use_pyref in (False, True):
        lanes = range(N) if not use_pyref else sorted({r[0] for r in listed})
        seen = sorted((i, st, k) for i in lanes for st, k in report_rejections(P, vk, doc["reports"][i], use_pyref))
        assert seen == listed, (seen, listed)
    for i in sorted({r[0] for r in listed}):
        rep = doc["reports"][i]
        args = [bytes.fromhex(rep[k]) for k in ("nonce", "public_share", "helper_input_share", "leader_prep_share")]
        assert rep["tamper"] == "" and rep["verdict"] == 0, i
        want = (0, bytes.fromhex(rep["prep_msg"]), bytes.fromhex(rep["out_share"]))
        assert orc.helper_prep(vk, *args) == want, i
        assert P.helper_prep(vk, *args) == want, i


# --------------------------------------------------------------------------- the hunt


def build_searcher(*defines):
    exe = os.path.join(tempfile.mkdtemp(prefix="reject_search_"), "reject_search")
    subprocess.run([os.environ.get("CC", "cc"), "-O3", "-march=native", "-mno-avx", "-pthread", *defines, "-o", exe,
                    os.path.join(ROOT, "tests", "csrc", "reject_search.c")], check=True)
    return exe


def preflight():
    """The searcher's three restatements against the oracle, in a second: a build that takes twelve set top
    bits for a hit finds some at once, and each must be where the C oracle's stream has them."""
    exe = build_searcher("-DREJECT_SEARCH_SELFTEST")
    C, M = R.Prio3("count"), pyref_of(dict(algo=O.SUMVEC_F64_MULTIPROOF, **MPA))
    head = lambda P, usage: bytes([8]) + P.dst(usage)  # noqa: E731

    def hits(*args):
        out = subprocess.run([exe, "4", "20", "0", *map(str, args)], check=True, capture_output=True, text=True).stdout
        got = [tuple(map(int, ln.split()[2:])) for ln in out.splitlines() if ln.startswith("HIT")]
        assert got, args
        return [(ctr.to_bytes(8, "little"), idx) for ctr, idx in got]

    def top12(stream, idx):
        return int.from_bytes(stream[8 * idx:8 * idx + 8], "little") >> 52 == 0xFFF

    tail, key, nonce, ph = b"selftest", b"k" * 24, bytes(range(16)), bytes(range(50, 82))
    for c, i in hits("ts", (head(C, "proof_share") + bytes(8) + tail + bytes([1, 1])).hex(), 9, 5, "0:5:1:0"):
        assert top12(O.xof_expand(c + tail, C.dst("proof_share"), bytes([1, 1]), 40), i)
    for c, i in hits("hmac", (bytes(8) + key).hex(), (head(M, "meas_share") + bytes([1])).hex(), "k", 0, 60, "0:60:2:0",
                     "0:60:2:1"):
        assert top12(O.xof_hmac_aes(c + key, M.dst("meas_share"), bytes([1]), 480), i)
    for c, i in hits("hmac", VK32.hex(), (head(M, "query_randomness") + bytes([8]) + bytes(8) + tail).hex(), "m", 10, 8,
                     "0:8:1:0"):
        assert top12(O.xof_hmac_aes(VK32, M.dst("query_randomness"), bytes([8]) + c + tail, 64), i)
    lmeas = list(range(100, 109))
    m1 = head(M, "joint_rand_part") + bytes([0]) + nonce + M.F.encode_vec(lmeas)
    for c, i in hits("hj", m1.hex(), head(M, "joint_rand_seed").hex(), ph.hex(),
                     (head(M, "joint_randomness") + bytes([8])).hex(), 8, "0:8:1:0"):
        seed = M.joint_rand_seed([M.joint_rand_part(0, c + bytes(24), lmeas, nonce), ph])
        assert top12(O.xof_hmac_aes(seed, M.dst("joint_randomness"), bytes([8]), 64), i)
    print("searcher self-test ok", flush=True)


def run_search(exe, classes, *args):
    """classes[i] names the class that COND i of the command line finds."""
    threads = str(min(16, os.cpu_count() or 1))
    cmd = [exe, threads, str(LOG2_BUDGET), "0", *map(str, args)]
    print("  ", " ".join(cmd), flush=True)
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    for line in out.splitlines():
        if line.startswith("HIT"):
            c, ctr, idx = map(int, line.split()[1:])
            FOUND[classes[c]] = (ctr, idx)
            print(f'    "{classes[c]}": ({ctr}, {idx}),', flush=True)
    for cls in classes:
        if cls not in FOUND:
            print(f"    {cls}: NOT FOUND within 2^{LOG2_BUDGET} tries")


def search(only=()):
    """Each step is one run of the searcher; `only` names the steps to redo (default: all)."""
    preflight()
    exe = build_searcher()
    C, M = R.Prio3("count"), pyref_of(dict(algo=O.SUMVEC_F64_MULTIPROOF, **MPA))
    z8 = bytes(8)

    def ts_msg(usage, seed, binder):  # TurboSHAKE128 input: len(dst) || dst || seed || binder
        return (bytes([8]) + C.dst(usage) + seed + binder).hex()

    def hm_msg(usage, binder):  # HMAC message (the seed is the key): len(dst) || dst || binder
        return (bytes([8]) + M.dst(usage) + binder).hex()

    def joint_args():
        # only the leader's blind moves, so the report stays an honest client's; all else is the
        # fixture's seeded report (which needs the measurement-stream hits of its other lanes first)
        name = MPA_NAME
        cfg, lanes = fixtures()[name]
        lane = next(i for i, (cls, _) in lanes.items() if cls == "mp_joint")
        _, meas, nonces, rands = inputs(name, cfg, lanes, skip=("mp_joint",))
        S, nonce, rand = M.S, nonces[lane].tobytes(), rands[lane].tobytes()
        hmeas = M.helper_meas_share(1, rand[:S])
        lmeas = [(a - b) % P64 for a, b in zip(M.valid.encode([int(x) for x in meas[lane]]), hmeas)]
        m1 = bytes([8]) + M.dst("joint_rand_part") + bytes([0]) + nonce + M.F.encode_vec(lmeas)
        ph = M.joint_rand_part(1, rand[4 * S:5 * S], hmeas, nonce)
        return ("hj", m1.hex(), (bytes([8]) + M.dst("joint_rand_seed")).hex(), ph.hex(),
                hm_msg("joint_randomness", bytes([M.PROOFS])), M.PROOFS, f"0:{M.PROOFS}:1:0")

    L, NP = MPA["length"], M.PROOFS
    nproof = min(256, M.valid.PROOF_LEN * NP)
    steps = {
        "count_meas": (["count_meas"], lambda: (
            "ts", ts_msg("meas_share", z8 + TAIL["count_meas"], bytes([1])), 9, 1, "0:1:1:0")),
        "count_proofs": (["count_proofs_4", "count_proofs_early"], lambda: (
            "ts", ts_msg("proof_share", z8 + TAIL["count_proofs_4"], bytes([1, 1])), 9, 5, "4:5:1:0", "0:4:1:0")),
        "count_query": (["count_query"], lambda: (
            "ts", ts_msg("query_randomness", VK16, bytes([1]) + z8 + TAIL["count_query"]), 9 + 16 + 1, 1, "0:1:1:0")),
        "mp_meas": (["mp_meas_last", "mp_meas_partial", "mp_meas_even", "mp_meas_odd"], lambda: (
            "hmac", (z8 + TAIL["mp_meas_even"]).hex(), hm_msg("meas_share", bytes([1])), "k", 0, 64,
            f"{L - 1}:{L}:1:0", "0:64:8:2", f"0:{L}:2:0", f"0:{L}:2:1")),
        "mp_proofs": (["mp_proofs"], lambda: (
            "hmac", (z8 + TAIL["mp_proofs"]).hex(), hm_msg("proof_share", bytes([NP, 1])), "k", 0, nproof,
            f"0:{nproof}:1:0")),
        "mp_query": (["mp_query"], lambda: (
            "hmac", VK32.hex(), hm_msg("query_randomness", bytes([NP]) + z8 + TAIL["mp_query"]), "m", 9 + 1, NP,
            f"0:{NP}:1:0")),
        "mp_joint": (["mp_joint"], joint_args),
    }
    for step, (classes, args) in steps.items():
        if only and step not in only:
            continue
        for cls in classes:
            FOUND.pop(cls, None)
        print(f"{step}:", flush=True)
        run_search(exe, classes, *args())
    print("FOUND = {")
    for k, v in FOUND.items():
        print(f'    "{k}": {v},')
    print("}")


if __name__ == "__main__":
    O.build()
    if "--search" in sys.argv[1:]:
        search(set(sys.argv[1:]) - {"--search"})
    for name, (cfg, lanes) in fixtures().items():
        missing = [cls for cls, _ in lanes.values() if cls not in FOUND]
        if missing:
            print(f"{name}: skipped, no hit recorded for {missing}")
            continue
        make(name, cfg, lanes)
