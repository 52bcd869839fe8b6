"""The leader's half of the framing rule (janus_amd/csrc/jx_wire.h) on the CPU: tests/csrc/hosttest_wire_leader.cpp, a
stand-alone program built with -fsanitize=address,undefined and run directly.

Response: wire_resp_walk + wire_resp_classify over seeded AggregationJobResp bodies written by janus_amd.messages.
Accept / reject must equal AggregationJobResp.decode for every body, the error offset must lie inside the field that
is wrong, the records must be what messages.py extracts, and the classification must be the branches of
aggregator.leader_process_helper_response. Request: a host replay of the kernels (select, scan, one wave's work per
loop iteration, the same jx_wire.h functions) against AggregationJobInitializeReq.encode(); the 64-bit total from
synthetic lengths; and the reference's own KATs (tests/golden/wire/dap_wire_kats.json) both ways."""
from __future__ import annotations

import itertools
import json
import os
import random
import struct
import subprocess

from janus_amd.messages import (AggregationJobInitializeReq, AggregationJobResp, CodecError, HpkeCiphertext,
                                PartialBatchSelector, PingPongMessage, PrepareError, PrepareInit, PrepareResp,
                                PrepareStepResult, ReportMetadata, ReportShare)

HERE = os.path.dirname(os.path.abspath(__file__))
PM = 16
CONTINUED, REJECTED, FINISHED, MESSAGE_MISMATCH = 0, 1, 2, 3
with open(os.path.join(HERE, "golden", "wire", "dap_wire_kats.json"), encoding="utf-8") as fh:
    KATS = json.load(fh)


def build_exe() -> str:
    src = os.path.join(HERE, "csrc", "hosttest_wire_leader.cpp")
    exe = os.path.join(HERE, "csrc", "hosttest_wire_leader")
    deps = [src] + [os.path.join(HERE, "..", "janus_amd", "csrc", h) for h in ("jx_wire.h", "jx_field.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"  # atomic: pytest-xdist workers may build concurrently
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", "-o", tmp, src], check=True)
        os.replace(tmp, exe)
    return exe


def run(mode: str, payload: bytes, tmp_path, out: bool = False):
    path = os.path.join(str(tmp_path), f"{mode}.bin")
    with open(path, "wb") as fh:
        fh.write(payload)
    args = [build_exe(), mode, path] + ([path + ".out"] if out else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    if out:
        with open(path + ".out", "rb") as fh:
            return fh.read()
    return r.stdout.splitlines()


# ----------------------------------------------------------------------------- the response


def run_resp(bodies, tmp_path, pm=PM) -> list[dict]:
    lines = run("resp", struct.pack("<I", len(bodies)) + b"".join(struct.pack("<IQ", pm, len(b)) + b for b in bodies),
                tmp_path)
    out = []
    for line in lines:
        head, *recs = line.split(" | ")
        t = head.split()
        out.append(dict(status=int(t[2]), err=int(t[3]), n=int(t[4]), recs=[tuple(int(x) for x in r.split()) for r in recs]))
    assert len(out) == len(bodies)
    return out


def variants(rnd) -> list[PrepareStepResult]:
    """One of every kind of result a response can carry."""
    v = [PrepareStepResult(0, message=PingPongMessage.finish(rnd.randbytes(k))) for k in (0, PM - 1, PM, PM + 1)]
    v.append(PrepareStepResult(0, message=PingPongMessage.initialize(rnd.randbytes(PM))))
    v.append(PrepareStepResult(0, message=PingPongMessage(1, rnd.randbytes(PM), rnd.randbytes(5))))
    v.append(PrepareStepResult(1))
    v += [PrepareStepResult(2, error=PrepareError(e)) for e in range(10)]
    return v


def resp_body(rnd, results) -> tuple[bytes, list[PrepareResp]]:
    resps = [PrepareResp(rnd.randbytes(16), r) for r in results]
    return AggregationJobResp(tuple(resps)).encode(), resps


def expected_resp_records(body: bytes, resps) -> list[tuple]:
    """(off, len, tag, pp_type, error, pm_off, pm_len, sh_len, class): each field found again by its own length; the
    class as leader_process_helper_response branches."""
    off, out = 4, []
    for p in resps:
        res, enc = p.result, p.encode()
        assert body[off:off + len(enc)] == enc
        if res.kind == 2:
            out.append((off, 18, 2, 0, int(res.error), 0, 0, 0, REJECTED))
        elif res.kind == 1:
            out.append((off, 17, 1, 0, 0, 0, 0, 0, FINISHED))
        else:
            m = res.message
            cls = CONTINUED if m.kind == PingPongMessage.FINISH and len(m.prep_msg) == PM else MESSAGE_MISMATCH
            pm_off = off + 22 + (4 if m.kind else 0)
            out.append((off, len(enc), 0, m.kind, 0, pm_off, len(m.prep_msg), len(m.prep_share), cls))
        off += len(enc)
    return out


def python_resp(body: bytes):
    try:
        return AggregationJobResp.decode(body)
    except CodecError:
        return None


def test_response_rule_under_sanitizers(tmp_path):
    rnd = random.Random(20240701)
    V = variants(rnd)
    valid: list[tuple[bytes, list]] = [resp_body(rnd, [])]
    valid += [resp_body(rnd, [r]) for r in V]
    tags = (V[2], V[6], V[10])  # Continue, Finished, Reject
    valid += [resp_body(rnd, list(mix)) for k in (2, 3) for mix in itertools.product(tags, repeat=k)]
    valid.append(resp_body(rnd, [V[(7 * i) % len(V)] for i in range(70)]))
    B: list[tuple[bytes, str, tuple | None]] = [(b, f"valid{k}", None) for k, (b, _) in enumerate(valid)]
    # the negatives, each with the span its error offset must lie in
    for b, resps in (valid[-1], resp_body(rnd, [V[2], V[5], V[11], V[2]])):
        recs = expected_resp_records(b, resps)
        vl = len(b) - 4
        B.append((b + b"\0", "after_vector", (len(b), len(b))))
        B.append((struct.pack(">I", vl + 1) + b[4:], "veclen+1", (0, 3)))
        B.append((struct.pack(">I", vl - 1) + b[4:], "veclen-1", (len(b) - 1, len(b) - 1)))
        for k in (1, 7, 200):
            B.append((struct.pack(">I", (1 << 32) - k) + b[4:], f"veclen=2^32-{k}", (0, 3)))
        conts = [i for i, r in enumerate(recs) if r[2] == 0]
        for which in {0, len(recs) // 2, len(recs) - 1} | {conts[0], conts[len(conts) // 2], conts[-1]}:
            off, ln, tag, pp = recs[which][:4]
            end = off + ln
            # (a cut at a message boundary is a valid, shorter response: it is no negative)
            cuts = {off + 16, off + 17} | ({off + 21, off + 22, off + 26, end - 1} if tag == 0 else set())
            for cut in sorted(c for c in cuts if c < end):  # truncated, the vector length made to fit
                short = b[:cut]
                B.append((struct.pack(">I", len(short) - 4) + short[4:], f"cut{cut}@{which}", (off, cut)))
                B.append((short, f"cut{cut}@{which}/veclen_kept", (0, 3)))
            B.append((b[:off + 16] + b"\x03" + b[off + 17:], f"tag3@{which}", (off + 16, off + 16)))
            if tag == 2:
                B.append((b[:off + 17] + b"\x0a" + b[off + 18:], f"error10@{which}", (off + 17, off + 17)))
            if tag != 0:
                continue
            M = ln - 21
            B.append((b[:off + 21] + b"\x03" + b[off + 22:], f"type3@{which}", (off + 21, off + 21)))
            for d in (-1, 1):  # the message length against its contents, then the inner length against the message
                B.append((b[:off + 17] + struct.pack(">I", M + d) + b[off + 21:], f"msglen{d:+d}@{which}", (off + 17, end)))
                inner = struct.unpack(">I", b[off + 22:off + 26])[0]
                B.append((b[:off + 22] + struct.pack(">I", (inner + d) & 0xFFFFFFFF) + b[off + 26:], f"inner{d:+d}@{which}", (off + 22, end)))
            for at in (off + 17, off + 22):
                B.append((b[:at] + b"\xff" * 4 + b[at + 4:], f"ff@{at}", (at, at + 3)))
                for k in (1, 5, 26):
                    B.append((b[:at] + struct.pack(">I", (1 << 32) - k) + b[at + 4:], f"2^32-{k}@{at}", (at, at + 3)))
            # a byte left over inside the message: the message one longer, the vector too
            grown = b[:off + 17] + struct.pack(">I", M + 1) + b[off + 21:end] + b"\x55" + b[end:]
            B.append((struct.pack(">I", vl + 1) + grown[4:], f"leftover@{which}", (end, end)))
    pool = [valid[-1][0], resp_body(rnd, [V[2], V[12], V[6], V[2], V[5]])[0]]
    for k in range(400):  # single-byte corruptions anywhere
        b = pool[k % 2]
        at = rnd.randrange(len(b))
        B.append((b[:at] + bytes([b[at] ^ (1 << rnd.randrange(8))]) + b[at + 1:], f"corrupt{k}@{at}", None))
    got = run_resp([b for b, _, _ in B], tmp_path)
    accepted = rejected = 0
    classes = set()
    for (body, name, span), g in zip(B, got):
        want = python_resp(body)
        assert (g["status"] == 0) == (want is not None), (name, g["status"], g["err"])
        if want is None:
            rejected += 1
            assert g["status"] == 1 and 0 <= g["err"] <= len(body), name
            if span is not None:
                assert span[0] <= g["err"] <= span[1], (name, g["err"], span)
            continue
        assert span is None, name  # every constructed negative is one
        accepted += 1
        assert g["n"] == len(want.prepare_resps), name
        assert g["recs"] == expected_resp_records(body, want.prepare_resps), name
        classes |= {r[8] for r in g["recs"]}
    print(f"{len(B)} bodies: {accepted} accepted, {rejected} rejected")
    assert accepted >= len(valid) and rejected > 250 and classes == {CONTINUED, REJECTED, FINISHED, MESSAGE_MISMATCH}


def test_response_kats(tmp_path):
    """The reference's own AggregationJobResp test vectors decode to their fields."""
    kats = KATS["aggregation_job_resp"]
    got = run_resp([bytes.fromhex(k["hex"]) for k in kats], tmp_path, pm=5)
    for k, g in zip(kats, got):
        body = bytes.fromhex(k["hex"])
        assert g["status"] == 0 and g["n"] == len(k["prepare_resps"])
        for want, r in zip(k["prepare_resps"], g["recs"]):
            off, ln, tag, pp, err, pm_off, pm_len, sh_len, cls = r
            assert body[off:off + 16].hex() == want["report_id"] and tag == want["kind"]
            if tag == 0:
                m = want["message"]
                assert pp == m["kind"] and body[pm_off:pm_off + pm_len].hex() == m["prep_msg"]
                assert sh_len == len(m["prep_share"]) // 2
                assert cls == (CONTINUED if pp == 2 and pm_len == 5 else MESSAGE_MISMATCH)
            elif tag == 2:
                assert err == want["error"] and cls == REJECTED
            else:
                assert cls == FINISHED


# ----------------------------------------------------------------------------- the request


def req_case(inits, verdicts, exclude, PS, LPS, query, param, batch_id) -> bytes:
    out = struct.pack("<IIIII", len(inits), PS, LPS, query, len(param)) + param + (batch_id or bytes(32))
    for p, v, x in zip(inits, verdicts, exclude):
        rs, ct = p.report_share, p.report_share.encrypted_input_share
        assert len(rs.public_share) == PS and len(p.message.prep_share) == LPS
        out += rs.metadata.report_id + struct.pack("<QBBBII", rs.metadata.time, ct.config_id, v, x,
                                                   len(ct.encapsulated_key), len(ct.payload))
        out += rs.public_share + ct.encapsulated_key + ct.payload + p.message.prep_share
    return out


def parse_req_out(blob: bytes, count: int):
    out, at = [], 0
    for _ in range(count):
        st = struct.unpack_from("<I", blob, at)[0]
        at += 4
        if st:
            out.append((st, None, None))
            continue
        ln = struct.unpack_from("<Q", blob, at)[0]
        body = blob[at + 8:at + 8 + ln]
        at += 8 + ln
        ns = struct.unpack_from("<I", blob, at)[0]
        out.append((0, body, list(struct.unpack_from(f"<{ns}I", blob, at + 4))))
        at += 4 + 4 * ns
    assert at == len(blob)
    return out


def make_init(rnd, PS, LPS, enc=32, pay=40) -> PrepareInit:
    return PrepareInit(ReportShare(ReportMetadata(rnd.randbytes(16), rnd.getrandbits(48)), rnd.randbytes(PS),
                                   HpkeCiphertext(rnd.randrange(256), rnd.randbytes(enc), rnd.randbytes(pay))),
                       PingPongMessage.initialize(rnd.randbytes(LPS)))


def test_request_replay_equals_the_codec(tmp_path):
    rnd = random.Random(20240702)
    cases, want = [], []

    def add(inits, verdicts, exclude, PS, LPS, fixed, param):
        bid = bytes(range(7, 39)) if fixed else None
        sel = PartialBatchSelector.fixed_size(bid) if fixed else PartialBatchSelector.time_interval()
        cases.append(req_case(inits, verdicts, exclude, PS, LPS, 2 if fixed else 1, param, bid))
        sent = [i for i in range(len(inits)) if verdicts[i] == 0 and not exclude[i]]
        want.append((AggregationJobInitializeReq(param, sel, tuple(inits[i] for i in sent)).encode(), sent))

    five = [make_init(rnd, 16, 24, enc=(32, 65)[i % 2], pay=40 + i) for i in range(5)]
    for mask in range(32):  # every send mask of a 5-report job, none sent included; the cause alternates
        send = [(mask >> i) & 1 for i in range(5)]
        verdicts = [0 if s or (mask + i) % 2 else 1 + i % 4 for i, s in enumerate(send)]
        exclude = [0 if s else int(verdicts[i] == 0) for i, s in enumerate(send)]
        add(five, verdicts, exclude, 16, 24, mask % 2 == 1, b"" if mask % 4 < 2 else b"param" * (mask % 3 + 1))
    for PS, LPS in ((0, 8), (0, 0), (16, 0), (48, 2864)):
        for encs in ((0, 32, 65, 65535), (65535,), (0,)):
            inits = [make_init(rnd, PS, LPS, enc=e, pay=(0, 1, 15, 16, 17, 300)[k % 6]) for k, e in enumerate(encs)]
            add(inits, [0] * len(inits), [0] * len(inits), PS, LPS, PS == 0, b"ab")
    add([], [], [], 16, 24, False, b"")
    add([], [], [], 16, 24, True, b"x" * 300)
    big = [make_init(rnd, 16, 24, enc=32 + i % 16, pay=(0, 1, 15, 16, 17, 50)[i % 6]) for i in range(130)]
    add(big, [int(rnd.random() < 0.25) for _ in big], [int(rnd.random() < 0.1) for _ in big], 16, 24, False, b"agg")
    got = parse_req_out(run("req", struct.pack("<I", len(cases)) + b"".join(cases), tmp_path, out=True), len(cases))
    for k, ((st, body, sent), (wbody, wsent)) in enumerate(zip(got, want)):
        assert st == 0 and sent == wsent, k
        assert body == wbody, k
    assert any(not w[1] for w in want) and len(want) >= 47


def test_request_kats(tmp_path):
    """The reference's AggregationJobInitializeReq vectors from their fields. The leader only ever writes Initialize
    messages, so the PrepareInits of a vector that carry one are encoded (the header, and each such PrepareInit, must be
    the vector's bytes at their place); a vector of Initialize messages alone is reproduced whole."""
    kats = KATS["aggregation_job_initialize_req"]
    cases, want, whole = [], [], 0
    for k in kats:
        inits = [PrepareInit(ReportShare(ReportMetadata(bytes.fromhex(p["report_id"]), p["time"]), bytes.fromhex(p["public_share"]),
                                         HpkeCiphertext(p["config_id"], bytes.fromhex(p["encapsulated_key"]),
                                                        bytes.fromhex(p["payload"]))),
                             PingPongMessage(p["message"]["kind"], bytes.fromhex(p["message"]["prep_msg"]),
                                             bytes.fromhex(p["message"]["prep_share"]))) for p in k["prepare_inits"]]
        bid = bytes.fromhex(k["batch_id"]) if k["batch_id"] else None
        sel = PartialBatchSelector.fixed_size(bid) if k["query_type"] == 2 else PartialBatchSelector.time_interval()
        param, full = bytes.fromhex(k["aggregation_parameter"]), bytes.fromhex(k["hex"])
        assert AggregationJobInitializeReq(param, sel, tuple(inits)).encode() == full
        whole += all(p.message.kind == 0 for p in inits)
        off = len(full) - sum(len(p.encode()) for p in inits)
        for p in inits:  # each Initialize PrepareInit alone: its lengths differ from its neighbours'
            if p.message.kind == 0:
                PS, LPS = len(p.report_share.public_share), len(p.message.prep_share)
                cases.append(req_case([p], [0], [0], PS, LPS, k["query_type"], param, bid))
                want.append((full[:off - 4], full[off:off + len(p.encode())]))
            off += len(p.encode())
    assert cases
    got = parse_req_out(run("req", struct.pack("<I", len(cases)) + b"".join(cases), tmp_path, out=True), len(cases))
    for (st, body, sent), (head, msg) in zip(got, want):
        assert st == 0 and sent == [0]
        assert body == head + struct.pack(">I", len(msg)) + msg
    print(f"{len(kats)} vectors, {len(cases)} Initialize PrepareInits, {whole} vectors of Initialize alone")


def test_total_is_64_bit_and_refuses(tmp_path):
    """wire_req_total from synthetic lengths, no buffers: a vector of exactly 2^32 bytes and one of 2^32 - 1 bytes plus
    one message are refused (3), 2^32 - 1 is not; a 65,536-byte key is refused (1), 65,535 is not; a payload of 2^32
    bytes is refused (2), 2^32 - 1 alone fits no u32 vector (3)."""
    PS, LPS, OK, KEY, PAY, VEC = 16, 24, 0, 1, 2, 3
    fixed = 44 + PS + LPS

    def case(encs, pays, query=1, param=5):
        n = len(pays)
        eo = [sum(encs[:i]) for i in range(n + 1)] if encs is not None else None
        po = [sum(pays[:i]) for i in range(n + 1)]
        blob = struct.pack("<QQQQII", n, PS, LPS, param, query, int(eo is not None))
        blob += b"".join(struct.pack("<Q", x) for x in (eo or []) + po)
        lens = [fixed + (encs[i] if encs is not None else 32) + pays[i] for i in range(n)]
        return blob, 4 + param + (33 if query == 2 else 1) + 4 + sum(lens)

    room = (1 << 32) - 1 - 2 * (fixed + 32)  # two messages' payloads that fill a vector of 2^32 - 1 bytes
    a, b = room // 2, room - room // 2
    table = [
        (case(None, [a, b]), OK), (case(None, [a, b + 1]), VEC), (case(None, [a, b, 0]), VEC),
        (case([32, 65535], [10, 10], query=2), OK), (case([32, 65536], [10, 10]), KEY), (case([65536], [0]), KEY),
        (case(None, [1 << 32]), PAY), (case(None, [(1 << 32) - 1]), VEC), (case(None, []), OK),
        (case([0, 0, 0], [0, 0, 0], param=0), OK),
    ]
    lines = run("total", struct.pack("<I", len(table)) + b"".join(c[0][0] for c in table), tmp_path)
    assert len(lines) == len(table)
    for k, (((_, total), status), line) in enumerate(zip(table, lines)):
        t = line.split()
        assert int(t[2]) == status, (k, line)
        if status == OK:
            assert int(t[3]) == total, (k, line)
