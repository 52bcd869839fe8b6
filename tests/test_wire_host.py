"""The framing rule of the aggregate-init request (janus_amd/csrc/jx_wire.h) on the CPU: tests/csrc/hosttest_wire.cpp, a
stand-alone program built with -fsanitize=address,undefined and run directly. It walks every seeded body written here
sequentially with the rule, and indexes it with a replay of the kernels' fast pass and fallback loop (one loop
iteration per lane); accept / reject must equal janus_amd.messages' decoder for every body, both ways of cutting must
agree (status, error offset, boundaries), and the records of an accepted body must be the fields messages.py extracts."""
from __future__ import annotations

import os
import random
import struct
import subprocess

import pytest

from janus_amd.messages import (AggregationJobInitializeReq, CodecError, HpkeCiphertext, PartialBatchSelector,
                                PingPongMessage, PrepareInit, ReportMetadata, ReportShare)

HERE = os.path.dirname(os.path.abspath(__file__))


def build_exe(sanitize: bool = True) -> str:
    """The program, with the sanitizers' runtimes linked into it (the tests of this file), or plain (sanitize=False:
    tests/test_gpu_wire.py asks it what the rule says, and sanitizers stay on the CPU tests)."""
    src = os.path.join(HERE, "csrc", "hosttest_wire.cpp")
    exe = os.path.join(HERE, "csrc", "hosttest_wire" if sanitize else "hosttest_wire_plain")
    deps = [src] + [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_wire.h", "jx_field.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
        subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + (san if sanitize else []) + ["-o", tmp, src], check=True)
        os.replace(tmp, exe)
    return exe


def run_bodies(bodies, tmp_path, sanitize: bool = True) -> list[dict]:
    """bodies: [(query type, bytes)] through the program; one parsed output line per body."""
    path = os.path.join(str(tmp_path), "bodies.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(bodies)))
        for q, b in bodies:
            fh.write(struct.pack("<IQ", q, len(b)) + b)
    r = subprocess.run([build_exe(sanitize), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = []
    for line in r.stdout.splitlines():
        head, *recs = line.split(" | ")
        t = head.split()
        d = dict(walk=(int(t[3]), int(t[4]), int(t[5])), index=(int(t[7]), int(t[8]), int(t[9])), iters=int(t[11]),
                 nfast=int(t[13]), same=int(t[15]))
        if d["walk"][0] == 0:
            d["hdr"] = (int(t[17]), int(t[18]), int(t[19]), bytes.fromhex(t[20]))
            d["recs"] = [tuple(int(x) for x in rec.split()) for rec in recs]
        out.append(d)
    assert len(out) == len(bodies)
    return out


def make_init(rnd, ps=16, enc=32, pay=40, kind=0, sh=24, cfg=None) -> PrepareInit:
    msg = PingPongMessage(kind, rnd.randbytes(7) if kind else b"", rnd.randbytes(sh) if kind < 2 else b"")
    return PrepareInit(ReportShare(ReportMetadata(rnd.randbytes(16), rnd.getrandbits(40)), rnd.randbytes(ps),
                                   HpkeCiphertext(rnd.randrange(256) if cfg is None else cfg, rnd.randbytes(enc),
                                                  rnd.randbytes(pay))), msg)


def request(inits, fixed=False, param=b"") -> bytes:
    sel = PartialBatchSelector.fixed_size(bytes(range(32))) if fixed else PartialBatchSelector.time_interval()
    return AggregationJobInitializeReq(param, sel, tuple(inits)).encode()


def expected_records(body: bytes, req: AggregationJobInitializeReq) -> list[tuple]:
    """The records messages.py's decode implies: each field found again by its own length."""
    off = 4 + len(req.aggregation_parameter) + len(req.partial_batch_selector.encode()) + 4
    out = []
    for p in req.prepare_inits:
        rs, ct, m = p.report_share, p.report_share.encrypted_input_share, p.message
        ps_off = off + 24 + 4
        enc_off = ps_off + len(rs.public_share) + 1 + 2
        pay_off = enc_off + len(ct.encapsulated_key) + 4
        msg_off = pay_off + len(ct.payload) + 4
        msg = m.encode()
        if m.kind == 0:
            pm_off = sh_off = msg_off + 5
        elif m.kind == 1:
            pm_off = msg_off + 5
            sh_off = pm_off + len(m.prep_msg) + 4
        else:
            pm_off = msg_off + 5
            sh_off = pm_off + len(m.prep_msg)
        ln = msg_off + len(msg) - off
        assert body[off:off + ln] == p.encode()
        out.append((off, ln, ps_off, len(rs.public_share), enc_off, len(ct.encapsulated_key), pay_off, len(ct.payload),
                    msg_off, len(msg), pm_off, len(m.prep_msg), sh_off, len(m.prep_share), ct.config_id, m.kind))
        off += ln
    return out


def field_boundaries(body: bytes, req) -> list[int]:
    """Every field boundary of the last message (offsets into body)."""
    r = expected_records(body, req)[-1]
    off, ln, ps_off, ps_len, enc_off, enc_len, pay_off, pay_len, msg_off, msg_len, pm_off, pm_len, sh_off, sh_len = r[:14]
    cuts = {off, off + 16, off + 24, ps_off, ps_off + ps_len, ps_off + ps_len + 1, enc_off, enc_off + enc_len, pay_off,
            pay_off + pay_len, msg_off, msg_off + 1, msg_off + 5, pm_off, pm_off + pm_len, sh_off, sh_off + sh_len}
    return sorted(c for c in cuts if c < len(body))


def length_fields(body: bytes, req) -> list[tuple[int, int]]:
    """(offset, width) of every length field of the body: the header's two and each message's."""
    out = [(0, 4), (4 + len(req.aggregation_parameter) + len(req.partial_batch_selector.encode()), 4)]
    for r in expected_records(body, req):
        off, ln, ps_off, ps_len, enc_off, enc_len, pay_off, pay_len, msg_off, msg_len, pm_off, pm_len, sh_off, sh_len, _, kind = r
        out += [(ps_off - 4, 4), (enc_off - 2, 2), (pay_off - 4, 4), (msg_off - 4, 4), (msg_off + 1, 4)]
        if kind == 1:
            out.append((sh_off - 4, 4))
    return out


def python_accepts(body: bytes, q: int):
    try:
        return AggregationJobInitializeReq.decode(body, q)
    except CodecError:
        return None


def all_bodies() -> list[tuple[int, bytes, str]]:
    rnd = random.Random(20240611)
    B: list[tuple[int, bytes, str]] = []
    valid = []
    for n in (0, 1, 2, 63, 64, 65):
        valid.append((request([make_init(rnd) for _ in range(n)], fixed=n % 2 == 0, param=b"p" * (n % 5)), f"uniform{n}",
                      2 if n % 2 == 0 else 1))
    valid.append((request([make_init(rnd, enc=32 if i % 2 else 65) for i in range(70)]), "mixed_enc", 1))
    valid.append((request([make_init(rnd, pay=40 + (i * 7) % 13) for i in range(70)]), "mixed_payload", 1))
    valid.append((request([make_init(rnd, pay=40 + i) for i in range(70)]), "growing_payload", 1))
    valid.append((request([make_init(rnd, enc=(32, 65, 65)[i % 3]) for i in range(70)]), "period3_enc", 1))
    valid.append((request([make_init(rnd, kind=i % 3) for i in range(9)]), "pingpong_types", 1))
    valid.append((request([make_init(rnd, ps=0 if i == 3 else 16) for i in range(6)]), "empty_ps", 1))
    valid.append((request([make_init(rnd)] * 66 + [make_init(rnd, pay=41)] + [make_init(rnd)] * 70), "uniform_one_odd", 1))
    for body, name, q in valid:
        B.append((q, body, name))
    for body, name, q in valid:
        req = AggregationJobInitializeReq.decode(body, q)
        if not req.prepare_inits:
            continue
        for cut in field_boundaries(body, req):  # truncated at every field boundary of the last message
            B.append((q, body[:cut], f"{name}/cut{cut}"))
        B.append((q, body + b"\0", name + "/trailing"))
        B.append((3 - q, body, name + "/wrong_query"))
        voff = 4 + len(req.aggregation_parameter) + len(req.partial_batch_selector.encode())
        vl = struct.unpack(">I", body[voff:voff + 4])[0]
        for d in (-1, 1):
            B.append((q, body[:voff] + struct.pack(">I", vl + d) + body[voff + 4:], f"{name}/veclen{d:+d}"))
        rec = expected_records(body, req)
        for which in {0, len(rec) // 2, len(rec) - 1}:
            r = rec[which]
            msg_off, msg_len = r[8], r[9]
            for d in (-1, 1):  # the inner message length against its contents, both ways
                B.append((q, body[:msg_off - 4] + struct.pack(">I", msg_len + d) + body[msg_off:], f"{name}/msglen{d:+d}@{which}"))
                B.append((q, body[:msg_off + 1] + struct.pack(">I", struct.unpack(">I", body[msg_off + 1:msg_off + 5])[0] + d)
                          + body[msg_off + 5:], f"{name}/inner{d:+d}@{which}"))
            B.append((q, body[:msg_off] + b"\x03" + body[msg_off + 1:], f"{name}/type3@{which}"))
        for off, w in length_fields(body, req)[:40] + length_fields(body, req)[-12:]:  # 0xFFFFFFFF in each length field
            B.append((q, body[:off] + b"\xff" * w + body[off + w:], f"{name}/ff@{off}"))
    # 400 random single-byte corruptions of length fields
    pool = [(b, q) for b, name, q in valid if name in ("uniform65", "mixed_enc", "pingpong_types", "uniform_one_odd", "uniform2")]
    for k in range(400):
        body, q = pool[k % len(pool)]
        req = AggregationJobInitializeReq.decode(body, q)
        off, w = rnd.choice(length_fields(body, req))
        at = off + rnd.randrange(w)
        B.append((q, body[:at] + bytes([body[at] ^ (1 << rnd.randrange(8))]) + body[at + 1:], f"corrupt{k}@{at}"))
    return B


def test_framing_rule_under_sanitizers(tmp_path):
    B = all_bodies()
    got = run_bodies([(q, b) for q, b, _ in B], tmp_path)
    accepted = rejected = fallback = 0
    for (q, body, name), g in zip(B, got):
        assert g["same"] == 1, (name, g["walk"], g["index"])
        req = python_accepts(body, q)
        assert (g["walk"][0] == 0) == (req is not None), (name, g["walk"])
        if req is None:
            rejected += 1
            if name.startswith("corrupt") or "/ff@" in name:  # a changed parameter length moves the query-type byte
                assert g["walk"][0] in (1, 2), name
            else:
                assert g["walk"][0] == (2 if name.endswith("/wrong_query") else 1), name
            assert 0 <= g["walk"][1] <= len(body), name
            continue
        accepted += 1
        fallback += g["iters"] > 0
        assert g["walk"][2] == len(req.prepare_inits), name
        assert g["recs"] == expected_records(body, req), name
        po, pl, has, bid = g["hdr"]
        assert body[po:po + pl] == req.aggregation_parameter, name
        assert (has, bid) == ((1, req.partial_batch_selector.batch_id) if q == 2 else (0, bytes(32))), name
        if name.startswith("uniform") and "/" not in name and name != "uniform_one_odd":
            assert g["iters"] == 0 and g["nfast"] == len(req.prepare_inits), name
        if name == "mixed_enc":
            assert g["iters"] == 2 and g["nfast"] == 1, g  # two alternating lengths: a wave's worth per iteration
        if name == "growing_payload":
            assert g["iters"] == 69 and g["nfast"] == 1, g  # one message per iteration: the fallback's worst case
        if name == "uniform_one_odd":
            assert g["nfast"] == 66 and 2 <= g["iters"] <= 4, g
    print(f"{len(B)} bodies: {accepted} accepted ({fallback} through the fallback loop), {rejected} rejected")
    assert accepted >= 13 and rejected > 400 and fallback >= 6


@pytest.mark.parametrize("field", range(4))
def test_lengths_near_2_32_do_not_wrap(tmp_path, field):
    """A length of 2^32 - k in a field makes a 32-bit sum of offset and length wrap to inside the body: rejected."""
    rnd = random.Random(field)
    body = request([make_init(rnd) for _ in range(3)])
    req = AggregationJobInitializeReq.decode(body, 1)
    r = expected_records(body, req)[1]
    off = (r[2] - 4, r[6] - 4, r[8] - 4, r[8] + 1)[field]
    bodies = [(1, body[:off] + struct.pack(">I", (1 << 32) - k) + body[off + 4:]) for k in range(1, 200)]
    for (q, b), g in zip(bodies, run_bodies(bodies, tmp_path)):
        assert python_accepts(b, q) is None and g["walk"][0] == 1 and g["same"] == 1
