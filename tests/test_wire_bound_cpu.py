"""The payload stage's item bound (gubernator_amd/csrc/guber_wire_parse.h wpl_item_bound: the host's walk of an RPC's top level BEFORE the
RPC joins a stage — the places it reserves there, the size of guber_wire_pool_response_bound(), the choice of the caller's own
evaluation) against the decoders that deliver the items afterwards, on tests/wire_shapes.py's structured payloads: unknown fields of
every kind and, above all, groups, which the decoders skip and the walk once stopped at.  A bound below the decoders' count overfills a
stage (other callers' RPCs are turned away with GUBER_E_WIRE_TOO_LARGE) and undersizes the caller's own buffer (GUBER_E_NOMEM after the
decisions have been applied); tests/test_gpu_wire_pool.py sends the same payloads through the stages."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import gubernator_amd as ga
import scenarios
import support
import wire_shapes
from gubernator_amd import wire as gw
from test_wire_cpu import NOW

WELL_FORMED = wire_shapes.well_formed()
MALFORMED = wire_shapes.malformed()


def test_the_shapes_are_what_they_are_built_as():
    """the host transcoder (pinned on the protobuf runtime by tests/test_wire_cpu.py) counts exactly the top-level records of every
    well-formed shape — what a group holds is no item — and turns every malformed sibling away; every kind is there at every place"""
    wb = gw.WireBatch(4096, 1 << 20)
    for label, payload in WELL_FORMED:
        wb.reset(NOW)
        assert wb.decode(payload, max_per_rpc=0) == (0, wire_shapes.n_records(label)), label
    for label, payload in MALFORMED:
        wb.reset(NOW)
        with pytest.raises(ga.GuberError) as ei:
            wb.decode(payload, max_per_rpc=0)
        assert ei.value.code == gw.E_WIRE_MALFORMED and len(wb) == 0, label
    labels = {label.rsplit("/n", 1)[0] for label, _ in WELL_FORMED}
    for kind in wire_shapes.ELEMENTS:
        assert {"%s/%s" % (kind, pos) for pos in wire_shapes.POSITIONS + ("long",)} <= labels, kind
    counts = {wire_shapes.n_records(label) for label, _ in WELL_FORMED if "/long/" not in label}
    assert counts == set(wire_shapes.COUNTS)
    for label, payload in WELL_FORMED:
        assert (len(payload) >= wire_shapes.WALK_MAX) == ("/long/" in label), label
    assert len(dict(WELL_FORMED)[wire_shapes.GROUP_LED_300]) == 7802
    wb.close()


def test_the_item_bound_agrees_with_the_decoders_under_asan_fuzz(tmp_path):
    """tools/wire_fuzz_asan.cpp with the shapes in a file: every shape as it is, then 300 000 structured chains and mutations of them
    through guber_wire_decode_requests, scan_toplevel and wpl_item_bound (-fsanitize=address,undefined, exact-size heap buffers) —
    scan_toplevel's verdict and count are the host transcoder's; wpl_item_bound(p, len, cap) >= min(count, cap) for cap 4 / 1000 / 4096
    on whatever scan_toplevel accepts, and == min(count, cap) below GUBER_WPL_WALK_MAX bytes.  (On the walk as it was — `else break` at
    wire types 3 / 4 — the same run reports 32 813 item bounds below the count.)"""
    shapes = tmp_path / "shapes.bin"
    with open(shapes, "wb") as f:
        for label, payload in WELL_FORMED:
            f.write(struct.pack("<II", len(payload), wire_shapes.n_records(label)) + payload)
        for label, payload in MALFORMED:
            f.write(struct.pack("<II", len(payload), 0xffffffff) + payload)
    exe = str(tmp_path / "wire_fuzz")
    root = support.ROOT
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-Wno-attributes", "-Wno-unknown-pragmas", "-I", os.path.join(root, "include"),
                    "-I", os.path.join(root, "tests", "hostsim", "fakehip"), os.path.join(root, "tools", "wire_fuzz_asan.cpp"), os.path.join(root, "gubernator_amd", "csrc", "wire.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, "300000", str(shapes)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "(%d from the file)" % (len(WELL_FORMED) + len(MALFORMED)) in out.stdout
    assert ": 0 item bounds below the count, 0 above it, 0 verdicts apart" in out.stdout and "no sanitizer report" in out.stdout


def _bound(L, payload):
    return L.guber_wire_pool_response_bound(payload, len(payload))


def test_the_response_bound_covers_the_worst_answers_to_every_shape():
    """guber_wire_pool_response_bound(p, len) >= the length of guber_wire_encode_responses' bytes when (a) every item answers status 1 and
    limit = remaining = reset_time = -1 (37 bytes an item: the longest answer without an error) and (b) every item answers the longest error
    text (tests/test_wire_peer_cpu.py's arrangement: the Gregorian one), in client mode (the wrapper quotes the item's key) and in peer mode"""
    L = gw._lib()
    L.guber_wire_pool_response_bound.argtypes = [C.c_char_p, C.c_size_t]
    L.guber_wire_pool_response_bound.restype = C.c_size_t
    longest = max(len(r["text"].encode()) for r in scenarios.load("peer_error_texts.json")["rows"])
    wb = gw.WireBatch(4096, 1 << 20)
    checked = 0
    for label, payload in WELL_FORMED:
        n = wire_shapes.n_records(label)
        assert n <= 4096
        bound = _bound(L, payload)
        for peer in (False, True):
            wb.reset(NOW)
            first, count = wb.decode(payload, max_per_rpc=0, peer=peer)
            assert count == n
            res = wb.result()
            col = lambda name, dt: np.ctypeslib.as_array(C.cast(getattr(res, name), C.POINTER(dt)), shape=(max(n, 1),))[:n]  # noqa: E731
            col("status", C.c_uint8)[:] = 1
            for name in ("limit", "remaining", "reset_time"):
                col(name, C.c_int64)[:] = -1
            col("err", C.c_uint8)[:] = 0
            plain = wb.encode(first, count, peer=peer)
            if not peer and "/middle/n60" not in label:           # (the n60 middles hold a request without a key: its answer is that error)
                assert len(plain) == 37 * n, label
            assert len(plain) <= bound, (label, peer, len(plain), bound)
            col("err", C.c_uint8)[:] = 3
            worst = wb.encode(first, count, peer=peer)
            if peer:
                assert len(worst) == n * (1 + 2 + 1 + 2 + longest), label
            assert len(worst) >= len(plain) and len(worst) <= bound, (label, peer, len(worst), bound)
            checked += 1
    assert checked == 2 * len(WELL_FORMED)
    wb.close()
