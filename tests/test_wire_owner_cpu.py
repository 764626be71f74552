"""guber_wire_encode_responses_owner (gubernator_amd/csrc/wire.cpp) against the protobuf runtime: GetRateLimitsResp bytes whose answers carry
metadata{"owner": <address>} wherever another rank owns the item.  The expected bytes are RateLimitResp messages built through
tests/pb_schema.py from the table of include/guber_wire.h, with the error texts written out here:
  1  pre-rejected, or owner_rank 0xFF       the client path's text, no metadata
  2  owner_rank == self_rank                the client path's text (wrap_errors honoured), no metadata
  3  plain, another owner (forwarded)       "Error in getLocalRateLimit: during workerPool.GetRateLimit: ..." (gubernator.go:523 around :600), metadata
  4  GLOBAL, another owner                  "Error in getGlobalRateLimit: during in getLocalRateLimit: during workerPool.GetRateLimit: ..."
                                            (gubernator.go:261, :416, :600), metadata
Address lengths 1, 11, 100, 118, 119, 127, 128 and 264 are where entry_len and addr_len take a second byte; with the 100-byte address the
answers' fields put the body on 127 and on 128 bytes, where the item's own length prefix does."""
import ctypes as C

import numpy as np
import pytest

import gubernator_amd as ga
from gubernator_amd import wire as gw
from pb_schema import PB
import wire_replay

NOW = 1_700_000_000_000
GLOBAL, GREGORIAN = 2, 4
GREG = "behavior DURATION_IS_GREGORIAN is set; but `Duration` is not a valid gregorian interval"
ALGO = "Invalid rate limit algorithm '7'"
TOO_LONG = "rate limit key too long"
LOCAL = "Error in getLocalRateLimit: during workerPool.GetRateLimit: "
GLOBAL_PREFIX = "Error in getGlobalRateLimit: during in getLocalRateLimit: during workerPool.GetRateLimit: "
ADDR_LENS = (1, 11, 100, 118, 119, 127, 128, 264)
E_GREG, E_ALGO, E_TOO_LONG = 3, 1, 7
I64_MAX = (1 << 63) - 1


def addr_of(n):
    return ("h" * n)[:max(n - 5, 0)] + ":8081"[-min(n, 5):]


def req(name, ukey, behavior=0, algorithm=0):
    return dict(name=name, unique_key=ukey, hits=1, limit=10, duration=60_000, algorithm=algorithm, behavior=behavior, burst=0, created_at=0)


def client_text(key, text, wrap):
    return f"Error while apply rate limit for '{key}': {text}" if wrap else text


class Case:
    """items: (request, owner_rank, (status, limit, remaining, reset_time), err code, expected text or None, expects metadata)"""

    def __init__(self):
        self.items = []

    def add(self, r, owner, fields=(0, 10, 9, NOW + 60_000), err=0, text=None, meta=False):
        self.items.append((r, owner, fields, err, text, meta))

    def run(self, addrs, self_rank, wrap, cap=None):
        wb = gw.WireBatch(len(self.items) + 1, 1 << 16)
        wb.reset(NOW)
        first, count = wb.decode(wire_replay.pb_request([it[0] for it in self.items]), max_per_rpc=0)
        assert (first, count) == (0, len(self.items))
        res, n = wb.result(), count
        col = lambda name, dt: np.ctypeslib.as_array(C.cast(getattr(res, name), C.POINTER(dt)), shape=(n,))  # noqa: E731
        for i, (_, _, f, err, _, _) in enumerate(self.items):
            col("status", C.c_uint8)[i], col("limit", C.c_int64)[i], col("remaining", C.c_int64)[i], col("reset_time", C.c_int64)[i] = f
            col("err", C.c_uint8)[i] = err
        try:
            return wb.encode_owner(0, n, [it[1] for it in self.items], self_rank, addrs, wrap_errors=wrap, cap=cap), wb
        except ga.GuberError:
            wb.close()
            raise

    def expected(self, addrs):
        m = PB["GetRateLimitsResp"]()
        for _, owner, f, _, text, meta in self.items:
            x = m.responses.add()
            if text is not None:
                x.error = text
            else:
                x.status, x.limit, x.remaining, x.reset_time = f
            if meta:
                x.metadata["owner"] = addrs[owner]
        return m.SerializeToString()


def table_case(wrap):
    """every row of the table, without an error and with each of them; self is rank 0, the other owner rank 1"""
    c = Case()
    for glob in (0, GLOBAL):
        for owner in (0, 1):
            remote = owner == 1
            tag = f"{'g' if glob else 'p'}{owner}"
            c.add(req("n", tag + "ok", glob), owner, meta=remote)
            for algo, word in ((0, "tokenBucket"), (1, "leakyBucket")):
                key = f"n_{tag}greg{algo}"
                text = (GLOBAL_PREFIX if glob else LOCAL) + f"Error in {word}: " + GREG if remote else client_text(key, GREG, wrap)
                c.add(req("n", f"{tag}greg{algo}", glob | GREGORIAN, algo), owner, err=E_GREG, text=text, meta=remote)
            key = f"n_{tag}algo"
            text = (GLOBAL_PREFIX if glob else LOCAL) + ALGO if remote else client_text(key, ALGO, wrap)
            c.add(req("n", tag + "algo", glob, 7), owner, err=E_ALGO, text=text, meta=remote)
    # row 1: pre-rejected items whatever the owner column says, and keys the ring cannot place
    c.add(req("n", ""), 1, text="field 'unique_key' cannot be empty")
    c.add(req("", "u"), 1, text="field 'namespace' cannot be empty")
    c.add(req("n", "", GLOBAL), 0xFF, text="field 'unique_key' cannot be empty")
    c.add(req("n", "long" * 30), 0xFF, err=E_TOO_LONG, text=client_text("n_" + "long" * 30, TOO_LONG, wrap))
    c.add(req("n", "unplaced"), 0xFF)
    # values: all zero, the int64 extremes (ten-byte varints)
    for owner in (0, 1):
        c.add(req("n", f"zero{owner}"), owner, fields=(0, 0, 0, 0), meta=owner == 1)
        c.add(req("n", f"max{owner}"), owner, fields=(1, I64_MAX, I64_MAX, I64_MAX), meta=owner == 1)
        c.add(req("n", f"neg{owner}"), owner, fields=(1, -1, -(1 << 63), -5), meta=owner == 1)
    return c


@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("n", ADDR_LENS)
def test_every_row_of_the_table_at_every_address_length(n, wrap):
    addrs = ["self:1", addr_of(n)]
    assert len(addrs[1]) == n
    c = table_case(wrap)
    got, wb = c.run(addrs, 0, wrap)
    want = c.expected(addrs)
    assert got == want
    m = PB["GetRateLimitsResp"]()
    m.ParseFromString(got)
    assert sum(1 for x in m.responses if x.metadata) == sum(1 for it in c.items if it[5]) > 0
    # seen from rank 1 the same owners put the metadata on the other half
    got1, wb1 = c.run(addrs, 1, wrap)
    m.ParseFromString(got1)
    assert all((dict(x.metadata) == {"owner": addrs[0]}) == (it[1] == 0 and it[0]["name"] != "" and it[0]["unique_key"] != "") for x, it in zip(m.responses, c.items))
    wb.close(); wb1.close()


def test_the_all_zero_answer_is_two_bytes_and_with_metadata_its_suffix():
    c = Case()
    c.add(req("n", "a"), 0, fields=(0, 0, 0, 0))
    c.add(req("n", "b"), 1, fields=(0, 0, 0, 0), meta=True)
    got, wb = c.run(["s", "o"], 0, 1)
    assert got == bytes([0x0a, 0x00]) + bytes([0x0a, 12, 0x32, 10, 0x0a, 5]) + b"owner" + bytes([0x12, 1]) + b"o" == c.expected(["s", "o"])
    wb.close()


def test_bodies_of_127_and_128_bytes_with_the_100_byte_address():
    """suffix = 1 + 1 + (2 + 5 + 1 + 1 + 100) = 111 bytes; fields of 16 bytes make the body 127 (one length byte), of 17 bytes 128 (two)"""
    addrs = ["s", addr_of(100)]
    for fields, body in (((1, 1 << 36, 1 << 36, 0), 127), ((1, 1 << 36, 1 << 42, 0), 128), ((1, 1 << 35, 1 << 36, 0), 127), ((1, -1, 1 << 42, 5), 111 + 2 + 11 + 8 + 2)):
        c = Case()
        c.add(req("n", "x"), 1, fields=fields, meta=True)
        got, wb = c.run(addrs, 0, 1)
        x = PB["RateLimitResp"](status=fields[0], limit=fields[1], remaining=fields[2], reset_time=fields[3])
        x.metadata["owner"] = addrs[1]
        assert x.ByteSize() == body
        assert got == c.expected(addrs) and len(got) == 1 + (1 if body < 128 else 2) + body
        wb.close()


def test_the_buffer_at_the_bound_at_the_length_and_one_below():
    """as guber_wire_encode_responses: cap >= the actual length is taken, one byte less is GUBER_E_NOMEM with the size needed"""
    addrs = ["self:1", addr_of(264)]
    c = table_case(1)
    want = c.expected(addrs)
    got, wb = c.run(addrs, 0, 1)                       # cap = guber_wire_encode_bound_owner
    arr = (C.c_char_p * 2)(*[a.encode() for a in addrs])
    bound = wb.L.guber_wire_encode_bound_owner(wb.h, 0, len(c.items), arr, 2)
    assert got == want and bound >= len(want) and bound == wb.L.guber_wire_encode_bound(wb.h, 0, len(c.items)) + len(c.items) * 277
    wb.close()
    got, wb = c.run(addrs, 0, 1, cap=len(want))
    assert got == want
    wb.close()
    with pytest.raises(ga.GuberError) as ei:
        c.run(addrs, 0, 1, cap=len(want) - 1)
    assert ei.value.code == ga.E_NOMEM and ei.value.needed == len(want)


def test_refusals():
    c = Case()
    c.add(req("n", "a"), 1, meta=True)

    def refused(addrs, self_rank=0, owners=None):
        if owners is not None:
            c.items[0] = (c.items[0][0], owners) + c.items[0][2:]
        with pytest.raises(ga.GuberError) as ei:
            c.run(addrs, self_rank, 1, cap=4096)
        assert ei.value.code == ga.E_INVALID_ARG
    refused(["s", ""])
    refused(["", "o"])
    refused(["s", None])
    refused(["s", "x" * 265])
    refused(["s", "o"], self_rank=2)
    refused(["s", "o"], owners=2)
    c.items[0] = (c.items[0][0], 1) + c.items[0][2:]
    wb = gw.WireBatch(4, 256)
    arr = (C.c_char_p * 2)(b"s", b"")
    assert wb.L.guber_wire_encode_bound_owner(wb.h, 0, 0, arr, 2) == 0
    wb.close()
    got, wb = c.run(["s", "x" * 264], 0, 1)
    assert got == c.expected(["s", "x" * 264])
    wb.close()
