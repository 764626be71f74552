"""Structured GetRateLimitsReq / GetPeerRateLimitsReq payloads: top-level chains of RateLimitReq records with the unusual but VALID
constructs of the protobuf wire format between them — unknown fields of every wire type, field numbers whose tags take two and five
bytes, field 1 with a wire type other than LEN, length varints that are not minimal, and proto2 groups (wire types 3 / 4), which every
protobuf runtime, the host transcoder (csrc/wire.cpp) and the device decoder (guber_kernels_wire.h scan_one) skip up to the matching
END_GROUP — and their malformed siblings, which all of them turn away whole.  Byte mutation of runtime-serialized payloads (the other
fuzzes of the wire front end) almost never produces a valid group; here every construct is built on purpose, as the first, a middle
and the last element of chains of 1 .. 4 records (an RPC its caller evaluates), 5, 60 and 300 (the stages), and once each in a payload
past 8 192 bytes (the host no longer walks it; the device walks it window by window, the construct lying across the windows' edge).

Shared by tests/test_wire_bound_cpu.py (the payload stage's host walk against the decoders, the response bound), tests/test_gpu_wire_pool.py
and tests/test_gpu_wire_peer.py (the same payloads through the stages).  No GPU, no engine: bytes and the protobuf runtime only.

well_formed() / malformed() return (label, payload) pairs; a well-formed label ends in "/n<records>" (n_records()): the number of
RateLimitReq records at the top level, which is the number of items the RPC has — what a group holds never becomes an item."""
import struct

import numpy as np

import wire_replay

COUNTS = (1, 2, 3, 4, 5, 60, 300)
POSITIONS = ("first", "middle", "last")
WALK_MAX = 8192                                       # GUBER_WPL_WALK_MAX = guber::WIRE_WIN: the host walks shorter payloads, the device's windows are this long
GROUP_LED_300 = "group_led_300_limit_2p62/n300"       # 300 requests of limit 2^62 behind an empty group: the response (29 bytes an item) is longer than the request (26)


def varint(v, pad=0):
    """v as a varint; pad > 0: that many bytes longer than needed (continuation bits over zero groups: valid, not minimal)"""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    for _ in range(pad):
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def tag(field, wt):
    return varint((field << 3) | wt)


def group(field, content=b""):
    return tag(field, 3) + content + tag(field, 4)


def req(key, limit=1000, algorithm=0, name="ws", duration=3_600_000):
    return dict(name=name, unique_key=key, hits=1, limit=limit, duration=duration, algorithm=algorithm, behavior=0)


def record(r):
    """one RateLimitReq as a top-level record: tag 0x0a, length, body — the runtime's own bytes"""
    return wire_replay.pb_request([r])


def _renumbered(rec, pad):
    """the record with its length varint `pad` bytes longer than needed"""
    assert rec[0] == 0x0a
    n, k = 0, 1
    while rec[k] & 0x80:
        n |= (rec[k] & 0x7f) << (7 * (k - 1)); k += 1
    n |= rec[k] << (7 * (k - 1)); k += 1
    return b"\x0a" + varint(n, pad) + rec[k:]


_SCALARS = tag(1, 0) + varint(300) + tag(2, 1) + bytes(range(8)) + tag(3, 5) + b"\x01\x02\x03\x04" + tag(4, 2) + varint(2) + b"ab"
_INNER = record(req("never_an_item", limit=1))

# every VALID element kind: name -> (bytes, RateLimitReq records it adds at the top level)
ELEMENTS = {
    # ---- plain
    "unknown_varint": (tag(15, 0) + varint(2**63 + 5), 0),
    "unknown_fixed64": (tag(2, 1) + struct.pack("<Q", 0x8081828384858687), 0),
    "unknown_fixed32": (tag(7, 5) + struct.pack("<I", 0x0a0b0c0a), 0),
    "unknown_len": (tag(9, 2) + varint(5) + b"\x0a\x03abc", 0),                 # (its content looks like a record)
    "unknown_len_empty": (tag(3, 2) + varint(0), 0),
    "tag_2_bytes": (tag(16, 0) + varint(1) + tag(2047, 2) + varint(3) + b"xyz", 0),
    "tag_5_bytes": (tag(2**25, 5) + b"\x0a\x00\x0a\x00" + tag(2**29 - 1, 2) + varint(2) + b"\x0a\x00", 0),
    "field_1_varint": (tag(1, 0) + varint(7), 0),
    "field_1_fixed64": (tag(1, 1) + b"\x0a\x01\x2a\x0a\x01\x2a\x0a\x00", 0),
    "field_1_fixed32": (tag(1, 5) + b"\x0a\x02\x0a\x00", 0),
    "unknown_len_padded_length": (tag(12, 2) + varint(4, pad=2) + b"\x0a\x02\x0a\x00", 0),
    "record_padded_length_1": (_renumbered(record(req("padded1")), 1), 1),      # (two bytes for a length below 128: the decoder's two-byte shortcut)
    "record_padded_length_3": (_renumbered(record(req("padded3")), 3), 1),      # (four bytes: by the book)
    # ---- groups
    "group_empty": (group(1), 0),                                               # 0b 0c
    "group_empty_field_19": (group(19), 0),                                     # 9b 01 9c 01
    "group_scalars": (group(2, _SCALARS), 0),
    "group_holding_records": (group(1, b"\x0a\x01\x2a") + group(5, _INNER + _INNER), 0),
    "group_nested_3": (group(2, tag(8, 0) + varint(1) + group(3, group(1, b"\x0a\x01\x2a") + _INNER) + group(2)), 0),
    "group_wide_field": (group(2**25, tag(1, 2) + varint(1) + b"\x2a") + group(300, group(2**29 - 1)), 0),
}
GROUP_KINDS = tuple(k for k in ELEMENTS if k.startswith("group"))


def n_records(label):
    """RateLimitReq records at the top level of a well-formed shape = the items its RPC has"""
    return int(label.rsplit("/n", 1)[1])


def _reqs(rng, n, with_error):
    """n short requests on few keys (RPC after RPC meets the same buckets, every fourth key runs dry on the way; a key keeps its
    algorithm); with_error: one with an empty unique_key (gubernator.go:208-217: an item error — the response goes through the host
    transcoder, key and text in it)"""
    out = [req("k%d" % k, limit=1000 if k % 4 else 30, algorithm=int(k) & 1) for k in rng.integers(0, 400, n)]
    if with_error:
        out[n // 3]["unique_key"] = ""
    return out


def chain(records, element, pos):
    at = {"first": 0, "middle": len(records) // 2, "last": len(records)}[pos]
    return b"".join(records[:at]) + element + b"".join(records[at:])


def well_formed(seed=0):
    """every element kind x {first, middle, last} x COUNTS records (a middle needs two records), each kind once across the edge of a
    payload's first 8 192 bytes, and GROUP_LED_300 -> [(label, payload)]"""
    rng = np.random.default_rng(seed)
    out = []
    for kind, (el, adds) in ELEMENTS.items():
        for pos in POSITIONS:
            for n in COUNTS:
                plain = n - adds
                if plain < (2 if pos == "middle" else 0):
                    continue
                recs = [record(r) for r in _reqs(rng, plain, with_error=(n == 60 and pos == "middle"))]
                out.append(("%s/%s/n%d" % (kind, pos, n), chain(recs, el, pos)))
    for kind, (el, adds) in ELEMENTS.items():
        recs, size, at = [], 0, WALK_MAX - max(1, len(el) // 2)   # the element lies across byte 8 192: it starts at `at`
        while at - size > 90:
            recs.append(record(_reqs(rng, 1, False)[0])); size += len(recs[-1])
        recs.append(record(req("x" * (1 + at - size - len(record(req("x")))))))   # (a key as long as it takes)
        assert size + len(recs[-1]) == at
        tail = [record(r) for r in _reqs(rng, 40, False)]
        payload = b"".join(recs) + el + b"".join(tail)
        assert len(payload) >= WALK_MAX and len(recs) + 40 + adds <= 1000
        out.append(("%s/long/n%d" % (kind, len(recs) + 40 + adds), payload))
    led = ELEMENTS["group_empty"][0] + b"".join(record(req("%03d" % i, limit=2**62, name="w", duration=60_000)) for i in range(300))
    assert len(led) < WALK_MAX
    out.append((GROUP_LED_300, led))
    assert len({label for label, _ in out}) == len(out)
    return out


def malformed(seed=0):
    """the groups' malformed siblings (and the reserved wire types) among 2 records (the caller's own evaluation would take them) and 20 (a
    stage): every decoder turns the whole message away"""
    rng = np.random.default_rng(1000 + seed)
    broken = {
        "group_unterminated": tag(3, 3) + tag(1, 0) + varint(1),
        "group_unterminated_nested": tag(3, 3) + group(4) + tag(4, 3),
        "group_ended_by_another_field": tag(1, 3) + tag(2, 4),
        "group_nested_ends_crossed": tag(1, 3) + tag(2, 3) + tag(1, 4) + tag(2, 4),
        "end_group_stray": tag(1, 4),
        "end_group_stray_field_9": tag(9, 4),
        "group_nested_70_deep": b"".join(tag(2 + k % 5, 3) for k in range(70)) + b"".join(tag(2 + k % 5, 4) for k in reversed(range(70))),
        "wire_type_6": tag(1, 6),
        "wire_type_7": tag(14, 7) + varint(0),
        "group_holding_wire_type_6": tag(2, 3) + tag(3, 6) + tag(2, 4),
    }
    out = []
    for kind, el in broken.items():
        for n in (2, 20):
            for pos in POSITIONS:
                recs = [record(r) for r in _reqs(rng, n, False)]
                out.append(("%s/%s/%d" % (kind, pos, n), chain(recs, el, pos)))
    return out
