"""The upload half of the framing rule (janus_amd/csrc/jx_wire.h) on the CPU: tests/csrc/hosttest_wire_upload.cpp, a
stand-alone program built with -fsanitize=address,undefined and run directly.

wire_parse_report over seeded Report bodies written by janus_amd.messages: accept / reject must equal Report.decode for
every body, the error offset must lie inside the field that is wrong, and the record must be what messages.py
extracts. wire_report_layout / wire_report_fixed_byte write the reference's own KATs (tests/golden/wire/
dap_report_kats.json) and seeded reports back byte for byte. wire_upload_check against the Python integers of
aggregator.handle_upload at every boundary. And a host replay of the kernels (parse, scan, gather; scan, pack: one
wave's work per loop iteration, the same jx_wire.h functions) against messages.py.

The helpers that say what a decode must give (expected_decode) and the classes of malformed bodies (malformed) are
shared with tests/test_gpu_wire_upload.py."""
from __future__ import annotations

import json
import os
import random
import struct
import subprocess

import numpy as np

from janus_amd.messages import CodecError, HpkeCiphertext, Report, ReportMetadata

HERE = os.path.dirname(os.path.abspath(__file__))
OK, MALFORMED, TOO_EARLY, TASK_EXPIRED, EXPIRED, ODD_PUBLIC_SHARE = range(6)
NO_ROW = 0xFFFFFFFF
KEY_NONE = 0xFF
U64 = (1 << 64) - 1
with open(os.path.join(HERE, "golden", "wire", "dap_report_kats.json"), encoding="utf-8") as fh:
    KATS = json.load(fh)["report"]


def build_exe() -> str:
    src = os.path.join(HERE, "csrc", "hosttest_wire_upload.cpp")
    exe = os.path.join(HERE, "csrc", "hosttest_wire_upload")
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


# ----------------------------------------------------------------------------- reports and what is wrong with them


def make_report(rnd, PS=32, lenc=32, lpay=50, henc=32, hpay=40, time=None, lcfg=None, hcfg=None) -> Report:
    return Report(ReportMetadata(rnd.randbytes(16), rnd.getrandbits(40) if time is None else time), rnd.randbytes(PS),
                  HpkeCiphertext(rnd.randrange(256) if lcfg is None else lcfg, rnd.randbytes(lenc), rnd.randbytes(lpay)),
                  HpkeCiphertext(rnd.randrange(256) if hcfg is None else hcfg, rnd.randbytes(henc), rnd.randbytes(hpay)))


def kat_report(k) -> Report:
    ct = lambda c: HpkeCiphertext(c["config_id"], bytes.fromhex(c["encapsulated_key"]), bytes.fromhex(c["payload"]))  # noqa: E731
    return Report(ReportMetadata(bytes.fromhex(k["report_id"]), k["time"]), bytes.fromhex(k["public_share"]),
                  ct(k["leader_encrypted_input_share"]), ct(k["helper_encrypted_input_share"]))


def elements(r: Report) -> list[tuple[str, int, int]]:
    """(name, start, end) of what the parser reads one after another: the 24-byte head, then every field with its
    length prefix, the config ids alone."""
    L, H = r.leader_encrypted_input_share, r.helper_encrypted_input_share
    out, at = [], 0
    for name, ln in (("head", 24), ("public_share", 4 + len(r.public_share)), ("leader_config_id", 1),
                     ("leader_enc", 2 + len(L.encapsulated_key)), ("leader_payload", 4 + len(L.payload)),
                     ("helper_config_id", 1), ("helper_enc", 2 + len(H.encapsulated_key)),
                     ("helper_payload", 4 + len(H.payload))):
        out.append((name, at, at + ln))
        at += ln
    return out


def expected_record(r: Report) -> tuple:
    """The record wire_parse_report must give for r.encode() at offset 0, each field found by its own length."""
    el = {name: (a, b) for name, a, b in elements(r)}
    L, H = r.leader_encrypted_input_share, r.helper_encrypted_input_share
    return (0, el["helper_payload"][1], el["public_share"][0] + 4, len(r.public_share), L.config_id, el["leader_enc"][0] + 2,
            len(L.encapsulated_key), el["leader_payload"][0] + 4, len(L.payload), H.config_id, el["helper_enc"][0] + 2,
            len(H.encapsulated_key), el["helper_payload"][0] + 4, len(H.payload))


def span_of_cut(r: Report, cut: int) -> tuple[int, int]:
    """A body cut at `cut`: the read that fails is the element the cut lies in (or the one that would start there)."""
    for _, a, b in elements(r):
        if a <= cut < b:
            return a, cut
    raise AssertionError(cut)


def malformed(rnd, r: Report) -> dict[str, list[tuple[bytes, tuple[int, int] | None]]]:
    """The classes of malformed bodies made from one valid report: name -> [(body, the span its error offset must lie
    in, None when only accept / reject is compared)]."""
    b = r.encode()
    el = elements(r)
    out: dict[str, list] = {k: [] for k in ("cut_at_boundary", "cut_before_boundary", "cut_after_boundary", "trailing_byte",
                                            "u16_overrun", "u32_overrun", "length_near_max", "empty_body", "short_body",
                                            "corrupt_length")}
    for _, a, _ in el[1:]:
        out["cut_at_boundary"].append((b[:a], span_of_cut(r, a)))
        out["cut_before_boundary"].append((b[:a - 1], span_of_cut(r, a - 1)))
        if a + 1 < len(b):
            out["cut_after_boundary"].append((b[:a + 1], span_of_cut(r, a + 1)))
    out["cut_before_boundary"].append((b[:-1], span_of_cut(r, len(b) - 1)))
    out["trailing_byte"].append((b + b"\0", (len(b), len(b))))
    for name, a, e in el:
        width = {"public_share": 4, "leader_enc": 2, "leader_payload": 4, "helper_enc": 2, "helper_payload": 4}.get(name)
        if width is None:
            continue
        ln = e - a - width
        fmt = ">H" if width == 2 else ">I"
        top = (1 << (8 * width)) - 1
        if ln + 1 <= top:  # a length that overruns by one: everything after it is read one byte late
            out["u16_overrun" if width == 2 else "u32_overrun"].append(
                (b[:a] + struct.pack(fmt, ln + 1) + b[a + width:], (a, len(b))))
        for k in (0, 1, 7):  # lengths near the maximum of the prefix: no sum of a position and a length may wrap
            if top - k > ln:
                # the field itself fails unless the rest of the body is long enough to be taken for it
                hi = a + width - 1 if top - k > len(b) - (a + width) else len(b)
                out["length_near_max"].append((b[:a] + struct.pack(fmt, top - k) + b[a + width:], (a, hi)))
    out["empty_body"].append((b"", (0, 0)))
    out["short_body"].append((b[:23], (0, 0)))
    a = el[4][1]  # the top byte of the leader payload's length
    out["corrupt_length"].append((b[:a] + bytes([b[a] ^ 0x40]) + b[a + 1:], (a, a + 3)))
    return out


def python_report(body: bytes):
    try:
        return Report.decode(body)
    except CodecError:
        return None


def python_check(t: int, now: int, skew: int, expiration, age) -> int:
    """aggregator.handle_upload's three checks, in Python integers."""
    if t > now + skew:
        return TOO_EARLY
    if expiration is not None and t > expiration:
        return TASK_EXPIRED
    if age is not None and now > t + age:
        return EXPIRED
    return OK


def expected_decode(bodies: list[bytes], PS: int, now: int, skew: int, expiration, age, key_first, key_second) -> dict:
    """What jx_upload_decode must give for these uploads, extracted by messages.py."""
    n = len(bodies)
    status, row_of = np.zeros(n, np.uint8), np.full(n, NO_ROW, np.uint32)
    ids_all, times_all = np.zeros((n, 16), np.uint8), np.zeros(n, np.uint64)
    acc = []
    for i, b in enumerate(bodies):
        r = python_report(b)
        if len(b) >= 24:
            ids_all[i], times_all[i] = np.frombuffer(b[:16], np.uint8), struct.unpack(">Q", b[16:24])[0]
        if r is None:
            status[i] = MALFORMED
            continue
        status[i] = python_check(r.metadata.time, now, skew, expiration, age)
        if status[i] == OK and len(r.public_share) != PS:
            status[i] = ODD_PUBLIC_SHARE
        if status[i] == OK:
            row_of[i] = len(acc)
            acc.append((i, r))
    j = b"".join
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)  # noqa: E731
    L = [r.leader_encrypted_input_share for _, r in acc]
    H = [r.helper_encrypted_input_share for _, r in acc]
    return dict(status=status, row_of=row_of, ids_all=ids_all, times_all=times_all, m=len(acc),
                index=np.array([i for i, _ in acc], np.uint32), ids=j(r.metadata.report_id for _, r in acc),
                times=np.array([r.metadata.time for _, r in acc], np.uint64), ps=j(r.public_share for _, r in acc),
                key_index=bytes(x for c in L for x in (key_first[c.config_id], key_second[c.config_id])),
                config_ids=bytes(c.config_id for c in H),
                offs=[off([c.encapsulated_key for c in L]), off([c.payload for c in L]), off([c.encapsulated_key for c in H]),
                      off([c.payload for c in H])],
                packed=[j(c.encapsulated_key for c in L), j(c.payload for c in L), j(c.encapsulated_key for c in H),
                        j(c.payload for c in H)])


def key_tables(rnd) -> tuple[bytes, bytes]:
    return bytes(rnd.choice((0, 1, 2, KEY_NONE)) for _ in range(256)), bytes(rnd.choice((3, KEY_NONE)) for _ in range(256))


def mixed_batch(rnd, n: int, PS: int, now: int) -> list[Report]:
    """n reports with encapsulated keys of 32, 65 and 0 bytes mixed and payloads of odd lengths, so every packed offset
    is arbitrary mod 16; times around `now`."""
    return [make_report(rnd, PS, (32, 65, 0)[i % 3], 37 + 5 * (i % 7), (65, 0, 32)[i % 3], 29 + 3 * (i % 5),
                        time=now - 50 + i) for i in range(n)]


# ----------------------------------------------------------------------------- the parse


def parse_lines(bodies, tmp_path) -> list[dict]:
    lines = run("parse", struct.pack("<I", len(bodies)) + b"".join(struct.pack("<Q", len(b)) + b for b in bodies), tmp_path)
    out = []
    for line in lines:
        head, *rec = line.split(" | ")
        t = head.split()
        out.append(dict(ok=int(t[2]), err=int(t[3]), rec=tuple(int(x) for x in rec[0].split()) if rec else None))
    assert len(out) == len(bodies)
    return out


def test_parse_equals_the_codec_under_sanitizers(tmp_path):
    rnd = random.Random(20241001)
    shapes = [dict(), dict(PS=0), dict(PS=0, lenc=0, lpay=0, henc=0, hpay=0), dict(lenc=65, henc=0), dict(PS=1, lpay=1, hpay=1),
              dict(PS=32, lenc=65535, lpay=300, henc=65535, hpay=17), dict(lpay=70000, hpay=66000)]
    valid = [make_report(rnd, **s) for s in shapes] + [kat_report(k) for k in KATS]
    B: list[tuple[bytes, str, tuple | None]] = [(r.encode(), f"valid{k}", None) for k, r in enumerate(valid)]
    for k, r in enumerate(valid):
        for name, cases in malformed(rnd, r).items():
            B += [(b, f"{name}@{k}", span) for b, span in cases]
    pool = [valid[0].encode(), valid[3].encode()]
    for k in range(400):  # single-byte corruptions anywhere
        b = pool[k % 2]
        at = rnd.randrange(len(b))
        B.append((b[:at] + bytes([b[at] ^ (1 << rnd.randrange(8))]) + b[at + 1:], f"corrupt{k}@{at}", None))
    got = parse_lines([b for b, _, _ in B], tmp_path)
    accepted = rejected = 0
    for (body, name, span), g in zip(B, got):
        want = python_report(body)
        assert bool(g["ok"]) == (want is not None), (name, g)
        if want is None:
            rejected += 1
            assert 0 <= g["err"] <= len(body), name
            if span is not None:
                assert span[0] <= g["err"] <= span[1], (name, g["err"], span)
            continue
        # every constructed negative is one, but for an overrun that another reading of the bytes happens to absorb
        assert span is None or "overrun" in name, name
        accepted += 1
        assert g["rec"] == expected_record(want), name
    print(f"{len(B)} bodies: {accepted} accepted, {rejected} rejected")
    assert accepted >= len(valid) + 100 and rejected > 400


def report_case(r: Report) -> bytes:
    L, H = r.leader_encrypted_input_share, r.helper_encrypted_input_share
    return (r.metadata.report_id + struct.pack("<QBBIIIII", r.metadata.time, L.config_id, H.config_id, len(r.public_share),
                                               len(L.encapsulated_key), len(L.payload), len(H.encapsulated_key), len(H.payload)) +
            r.public_share + L.encapsulated_key + L.payload + H.encapsulated_key + H.payload)


def test_kats_both_ways_and_written_reports(tmp_path):
    """Both KATs parse into their fields and are written back byte for byte by the layout and fixed-byte functions; so
    are seeded reports of every shape, a time and lengths with every byte set among them."""
    rnd = random.Random(20241002)
    got = parse_lines([bytes.fromhex(k["hex"]) for k in KATS], tmp_path)
    for k, g in zip(KATS, got):
        body = bytes.fromhex(k["hex"])
        assert g["ok"] == 1
        off, ln, ps_off, ps_len, lcfg, le_off, le_len, lp_off, lp_len, hcfg, he_off, he_len, hp_off, hp_len = g["rec"]
        L, H = k["leader_encrypted_input_share"], k["helper_encrypted_input_share"]
        assert (off, ln) == (0, len(body)) and body[:16].hex() == k["report_id"]
        assert struct.unpack(">Q", body[16:24])[0] == k["time"] and body[ps_off:ps_off + ps_len].hex() == k["public_share"]
        assert (lcfg, body[le_off:le_off + le_len].hex(), body[lp_off:lp_off + lp_len].hex()) == \
            (L["config_id"], L["encapsulated_key"], L["payload"])
        assert (hcfg, body[he_off:he_off + he_len].hex(), body[hp_off:hp_off + hp_len].hex()) == \
            (H["config_id"], H["encapsulated_key"], H["payload"])
    reports = [kat_report(k) for k in KATS]
    reports += [make_report(rnd, PS, le, lp, he, hp, time=t) for PS, le, lp, he, hp, t in (
        (0, 0, 0, 0, 0, 0), (32, 32, 50, 32, 40, U64), (0x0405, 0x0607, 0x010203, 0x0809, 0x010a0b, 0x0102030405060708),
        (1, 65535, 15, 1, 16, 1), (16, 31, 17, 33, 47, 1 << 63))]
    blob = run("write", struct.pack("<I", len(reports)) + b"".join(report_case(r) for r in reports), tmp_path, out=True)
    at = 0
    for k, r in enumerate(reports):
        ln = struct.unpack_from("<Q", blob, at)[0]
        assert blob[at + 8:at + 8 + ln] == r.encode(), k
        at += 8 + ln
    assert at == len(blob)
    assert blob[8:8 + len(KATS[0]["hex"]) // 2].hex() == KATS[0]["hex"]  # the KAT's own hex, not only its re-encoding


def test_upload_check_at_every_boundary(tmp_path):
    """time == the limit passes and limit + 1 fails, for each of the three; precedence when two fail; both sums where
    they overflow 64 bits (the saturated sum decides as Python's unbounded one)."""
    now, skew, exp, age = 1_700_000_000, 300, 1_700_000_100, 86_400
    table = [
        (now + skew, now, skew, None, None), (now + skew + 1, now, skew, None, None),
        (exp, now, skew, exp, None), (exp + 1, now, skew, exp, None),
        (now - age, now, skew, None, age), (now - age - 1, now, skew, None, age),
        (now, now, 0, now, 0), (now + 1, now, 0, now, 0), (now - 1, now, 0, now, 0),
        (now + skew + 1, now, skew, now, age),          # too early and past the expiration: too early first
        (exp + 1, now + 2 * age, skew, exp, age),       # past the expiration and expired: the expiration first
        (now - age - 1, now, skew, now - 2 * age, age),  # the same, the other way round
        (0, 0, 0, None, None), (0, 0, 0, 0, 0), (U64, 0, U64, None, None), (U64, 1, U64 - 1, U64, 0),
        (U64, U64, 5, None, None),                     # now + skew overflows: nothing is too early
        (U64 - 10, U64, 0, None, 100),                 # time + age overflows: not expired
        (U64 - 10, U64, 0, None, 10), (U64 - 10, U64, 0, None, 9),  # the sum is exactly 2^64 - 1; one short of it
        (5, U64, U64, 4, U64), (U64, U64 - 1, 0, None, None), (U64, U64 - 1, 1, U64 - 1, None),
    ]
    blob = struct.pack("<I", len(table))
    for t, nw, sk, e, a in table:
        blob += struct.pack("<QQQIQIQ", t, nw, sk, e is not None, e or 0, a is not None, a or 0)
    lines = run("check", blob, tmp_path)
    got = [int(line.split()[2]) for line in lines]
    want = [python_check(*row) for row in table]
    assert got == want
    assert want[:6] == [OK, TOO_EARLY, OK, TASK_EXPIRED, OK, EXPIRED] and want[9:12] == [TOO_EARLY, TASK_EXPIRED, TASK_EXPIRED]
    assert set(want) == {OK, TOO_EARLY, TASK_EXPIRED, EXPIRED}


# ----------------------------------------------------------------------------- the kernels, replayed


def decode_blob(bodies, PS, parts, now, skew, expiration, age, kf, ks) -> bytes:
    off = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype("<u8")
    body = b"".join(bodies)
    return (struct.pack("<IIIQQIQIQ", len(bodies), PS, parts, now, skew, expiration is not None, expiration or 0,
                        age is not None, age or 0) + kf + ks + off.tobytes() + struct.pack("<Q", len(body)) + body)


def parse_decode_out(blob: bytes, n: int, PS: int) -> dict:
    at = 0

    def take(k):
        nonlocal at
        at += k
        return blob[at - k:at]

    out = dict(status=np.frombuffer(take(n), np.uint8), row_of=np.frombuffer(take(4 * n), "<u4"),
               ids_all=np.frombuffer(take(16 * n), np.uint8).reshape(n, 16), times_all=np.frombuffer(take(8 * n), "<u8"))
    m = out["m"] = struct.unpack("<Q", take(8))[0]
    out.update(index=np.frombuffer(take(4 * m), "<u4"), ids=take(16 * m), times=np.frombuffer(take(8 * m), "<u8"),
               ps=take(PS * m), key_index=take(2 * m), config_ids=take(m), offs=[], packed=[])
    for _ in range(4):
        o = np.frombuffer(take(8 * (m + 1)), "<u8")
        out["offs"].append(o)
        out["packed"].append(take(int(o[-1])))
    assert at == len(blob)
    return out


def assert_decode_equal(got: dict, want: dict):
    for k in ("status", "row_of", "ids_all", "times_all", "index", "times"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["m"] == want["m"]
    for k in ("ids", "ps", "key_index", "config_ids"):
        assert bytes(got[k]) == bytes(want[k]), k
    for f in range(4):
        np.testing.assert_array_equal(got["offs"][f], want["offs"][f], err_msg=f"offs{f}")
        assert bytes(got["packed"][f]) == bytes(want["packed"][f]), f"packed{f}"


def test_decode_replay_equals_the_codec(tmp_path):
    rnd = random.Random(20241003)
    now, skew, exp, age, PS = 1_700_000_000, 10, 1_700_000_005, 40, 32
    kf, ks = key_tables(rnd)
    reports = mixed_batch(rnd, 70, PS, now)
    base = [r.encode() for r in reports]
    base[3] = make_report(rnd, PS + 1, time=now).encode()
    base[5] = make_report(rnd, 0, time=now).encode()
    bad = malformed(rnd, reports[37])
    cases = [[c[k % len(c)][0] for c in bad.values()][k] for k in range(len(bad))]
    seen = set()
    for k, wrong in enumerate(cases + [None]):
        bodies = list(base)
        if wrong is not None:
            bodies[37] = wrong
        for parts in (1, 3):
            got = parse_decode_out(run("decode", decode_blob(bodies, PS, parts, now, skew, exp, age, kf, ks), tmp_path, out=True),
                                   len(bodies), PS)
            want = expected_decode(bodies, PS, now, skew, exp, age, kf, ks)
            assert_decode_equal(got, want)
        seen |= set(want["status"].tolist())
        assert want["status"][37] == (MALFORMED if wrong is not None else OK) and want["status"][3] == ODD_PUBLIC_SHARE
        assert want["status"][36] == OK and want["status"][38] == OK
    assert seen == {OK, MALFORMED, TOO_EARLY, TASK_EXPIRED, EXPIRED, ODD_PUBLIC_SHARE}
    # no uploads; none accepted; no limits
    for bodies, e, a in (([], exp, age), ([b"", b"x" * 23, base[3]], exp, age), (base, None, None)):
        got = parse_decode_out(run("decode", decode_blob(bodies, PS, 2, now, skew, e, a, kf, ks), tmp_path, out=True), len(bodies), PS)
        assert_decode_equal(got, expected_decode(bodies, PS, now, skew, e, a, kf, ks))


def test_pack_replay_equals_the_codec(tmp_path):
    rnd = random.Random(20241004)
    for n, PS, le, lc, he, hc, has_status, parts in ((70, 32, 32, 150, 32, 70, 1, 1), (70, 0, 32, 55, 65, 38, 1, 3),
                                                    (5, 32, 0, 0, 0, 0, 0, 2), (0, 32, 32, 150, 32, 70, 1, 1),
                                                    (3, 32, 65535, 17, 1, 4099, 0, 4)):
        reports = [make_report(rnd, PS, le, lc, he, hc, lcfg=7, hcfg=201) for _ in range(n)]
        status = [int(has_status and i in (0, 37, n - 1)) for i in range(n)]
        blob = struct.pack("<IIIIIIBBII", n, PS, le, lc, he, hc, 7, 201, has_status, parts)
        for r, s in zip(reports, status):
            L, H = r.leader_encrypted_input_share, r.helper_encrypted_input_share
            blob += (r.metadata.report_id + struct.pack("<QB", r.metadata.time, s) + r.public_share + L.encapsulated_key +
                     L.payload + H.encapsulated_key + H.payload)
        out = run("pack", blob, tmp_path, out=True)
        offs = np.frombuffer(out[:8 * (n + 1)], "<u8")
        enc = [b"" if s else r.encode() for r, s in zip(reports, status)]
        np.testing.assert_array_equal(offs, np.concatenate([[0], np.cumsum([len(x) for x in enc])]).astype(np.uint64))
        assert out[8 * (n + 1):] == b"".join(enc)
