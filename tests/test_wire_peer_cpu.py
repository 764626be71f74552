"""CPU tests of the peer mode of the wire front end (include/guber_wire.h guber_wire_decode_peer_requests /
guber_wire_encode_peer_responses): V1Instance.GetPeerRateLimits (gubernator.go:462-539) takes a GetPeerRateLimitsReq without the client
RPC's validation, ORs DRAIN_OVER_LIMIT into forwarded GLOBAL items and words its errors differently.  The decode is checked against a
model written here from the protobuf messages and those rules, the error texts against tests/golden/peer_error_texts.json (written by hand
from the reference), the client mode against the bytes it has always produced — and tests/test_gpu_wire_peer.py runs against the CPU build of
the engine, under AddressSanitizer, where k_wire_fill's peer branch is watched access by access."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gubernator_amd as ga
import scenarios
import support
import wire_replay
from gubernator_amd import wire as gw
from pb_schema import PB
from test_wire_cpu import NOW, check_decoded, rand_reqs

GLOBAL, DRAIN = 2, 32


def peer_model(m, now):
    """what GetPeerRateLimits makes of the parsed message, item by item (gubernator.go:499-520, client.go:39)"""
    out = []
    for q in m.requests:
        out.append(dict(key=(q.name + "_" + q.unique_key).encode(), hits=q.hits, limit=q.limit, duration=q.duration, burst=q.burst,
                        algorithm=q.algorithm if q.algorithm in (0, 1) else 255, algo_raw=q.algorithm,
                        behavior=q.behavior | (DRAIN if q.behavior & GLOBAL else 0),
                        created_at=q.created_at if q.HasField("created_at") and q.created_at else now, is_owner=1))
    return out


def check_peer_decoded(arr, base, model):
    for j, w in enumerate(model):
        i = base + j
        assert arr["keys"][i] == w["key"], (i, w)
        for f in ("hits", "limit", "duration", "burst", "algorithm", "behavior", "created_at", "is_owner"):
            assert arr[f][i] == w[f], (f, i, w, arr[f][i])


def test_peer_decode_matches_a_model_of_the_peer_rpc():
    """every field; empty name, empty unique_key, both; GLOBAL with and without DRAIN_OVER_LIMIT already set; several payloads in one batch,
    client ones between them (the two modes do not leak into each other)"""
    rng = np.random.default_rng(21)
    wb = gw.WireBatch(max_items=8192, max_key_bytes=1 << 19)
    wb.reset(NOW)
    fixed = [dict(name=n, unique_key=u, hits=3, limit=10, duration=1000, algorithm=a, behavior=b, burst=4, created_at=c)
             for n, u in (("", ""), ("n", ""), ("", "u"), ("n", "u")) for a in (0, 1, 7) for b in (0, GLOBAL, GLOBAL | DRAIN, DRAIN, GLOBAL | 8, 1 | 16)
             for c in (0, NOW - 77)]
    slices = []
    total = 0
    for rpc in range(14):
        reqs = fixed if rpc == 0 else rand_reqs(rng, int(rng.integers(0, 300)))
        peer = rpc % 3 != 2
        payload = wire_replay.pb_request(reqs, peer=peer)
        m = PB["GetPeerRateLimitsReq"]()
        m.ParseFromString(payload)
        first, count = wb.decode(payload, max_per_rpc=1000, peer=peer, is_owner=False)
        assert (first, count) == (total, len(reqs))
        slices.append((first, reqs, peer_model(m, NOW) if peer else None))
        total += count
    arr = wb.arrays()
    pre = wb.pre_errors()
    seen = dict(empty_name=0, empty_ukey=0, both=0, global_plain=0, global_drain=0)
    for first, reqs, model in slices:
        if model is None:
            check_decoded(arr, first, reqs, NOW, is_owner=0)      # the client decode, untouched (is_owner as passed)
            assert pre[first:first + len(reqs)].tolist() == [1 if not r["unique_key"] else 2 if not r["name"] else 0 for r in reqs]
            continue
        check_peer_decoded(arr, first, model)
        assert not pre[first:first + len(reqs)].any()             # no validation on this path (gubernator.go:208-217 is client-only)
        for r, w in zip(reqs, model):
            seen["both"] += not r["name"] and not r["unique_key"]
            seen["empty_name"] += not r["name"] and bool(r["unique_key"])
            seen["empty_ukey"] += bool(r["name"]) and not r["unique_key"]
            seen["global_plain"] += r["behavior"] & (GLOBAL | DRAIN) == GLOBAL
            seen["global_drain"] += r["behavior"] & (GLOBAL | DRAIN) == GLOBAL | DRAIN
            assert (w["behavior"] & DRAIN) == (DRAIN if r["behavior"] & (GLOBAL | DRAIN) else 0)
    assert min(seen.values()) >= 6, seen
    assert arr["keys"][0] == b"_" and arr["keys"][36] == b"n_" and arr["keys"][72] == b"_u" and arr["keys"][108] == b"n_u"
    # Gregorian items are precomputed on this path as on the client's
    wb.reset(NOW)
    wb.decode(wire_replay.pb_request([dict(name="g", unique_key="", hits=1, limit=10, duration=d, algorithm=0, behavior=4, burst=0) for d in (0, 3, 99)], peer=True), peer=True)
    a2 = wb.arrays()
    for i, d in enumerate((0, 3, 99)):
        assert (a2["greg_expire"][i], a2["greg_duration"][i]) == support.gregorian(NOW, d)
    wb.close()


def test_a_peer_rpc_of_1001_items_is_too_large_and_appends_nothing():
    rng = np.random.default_rng(4)
    big = wire_replay.pb_request(rand_reqs(rng, 1001), peer=True)
    wb = gw.WireBatch(4096, 1 << 18)
    wb.reset(NOW)
    wb.decode(wire_replay.pb_request(rand_reqs(rng, 5), peer=True), max_per_rpc=1000, peer=True)
    with pytest.raises(ga.GuberError) as ei:
        wb.decode(big, max_per_rpc=1000, peer=True)
    assert ei.value.code == gw.E_WIRE_TOO_LARGE and len(wb) == 5     # the same code as the client RPC's; the caller picks the text
    with pytest.raises(ga.GuberError) as ei:
        wb.decode(big[:-2], max_per_rpc=1000, peer=True)
    assert ei.value.code == gw.E_WIRE_MALFORMED and len(wb) == 5
    assert wb.decode(big, max_per_rpc=0, peer=True) == (5, 1001)
    wb.close()


def test_peer_error_texts_for_every_item_error_code():
    """tests/golden/peer_error_texts.json, one row per code of guber_item_strerror (and both algorithms where the text depends on it): the
    response carries {error} only, byte-identical to the protobuf runtime's GetPeerRateLimitsResp"""
    table = scenarios.load("peer_error_texts.json")
    rows = table["rows"]
    L = ga.lib()
    L.guber_item_strerror.restype = C.c_char_p
    codes = [c for c in range(1, 256) if L.guber_item_strerror(c) != L.guber_item_strerror(255)]
    assert sorted({r["code"] for r in rows}) == codes == list(range(1, 8))       # every code the engine can report has a row
    reqs = [dict(name="n", unique_key="k%d" % i, hits=1, limit=10, duration=1000, algorithm=r["algorithm"], behavior=0) for i, r in enumerate(rows)]
    reqs.append(dict(name="n", unique_key="fine", hits=1, limit=10, duration=1000, algorithm=0, behavior=0))
    wb = gw.WireBatch(64, 4096)
    wb.reset(NOW)
    first, count = wb.decode(wire_replay.pb_request(reqs, peer=True), peer=True)
    n = count
    res = wb.result()
    err = np.ctypeslib.as_array(C.cast(res.err, C.POINTER(C.c_uint8)), shape=(n,))
    for name in ("status", "limit", "remaining", "reset_time"):
        dt = C.c_uint8 if name == "status" else C.c_int64
        np.ctypeslib.as_array(C.cast(getattr(res, name), C.POINTER(dt)), shape=(n,))[:] = 1 if name == "status" else 7
    err[:] = [r["code"] for r in rows] + [0]
    want = PB["GetPeerRateLimitsResp"]()
    for r in rows:
        want.rate_limits.add(error=r["text"])
    want.rate_limits.add(status=1, limit=7, remaining=7, reset_time=7)
    got = wb.encode(first, count, peer=True)
    parsed = PB["GetPeerRateLimitsResp"]()
    parsed.ParseFromString(got)
    for r, x in zip(rows, parsed.rate_limits):
        assert x.error == r["text"], (r["code"], r["lines"], x.error)
    assert got == want.SerializeToString(deterministic=True)
    assert len(got) <= L.guber_wire_encode_bound(wb.h, first, count)
    assert table["too_large"]["text"] == "'PeerRequest.rate_limits' list too large; max size is '1000'"
    assert table["too_large"]["text"].replace("'1000'", "'%d'") in open(os.path.join(support.ROOT, "go", "wire_server.go")).read()
    wb.close()


def test_the_response_bounds_cover_the_longest_peer_text():
    """guber_wire_pool_response_bound / guber_wire_encode_bound against an RPC whose every item answers the longest peer text (82 bytes of
    wrappers around the 92 of the Gregorian one), with keys of one byte: no key pads the bound"""
    L = gw._lib()
    L.guber_wire_pool_response_bound.argtypes = [C.c_char_p, C.c_size_t]
    L.guber_wire_pool_response_bound.restype = C.c_size_t
    longest = max(len(r["text"].encode()) for r in scenarios.load("peer_error_texts.json")["rows"])
    for n in (1, 4, 5, 1000):
        payload = wire_replay.pb_request([dict(name="", unique_key="", hits=1, limit=1, duration=99, algorithm=1, behavior=4)] * n, peer=True)
        wb = gw.WireBatch(1024, 4096)
        wb.reset(NOW)
        first, count = wb.decode(payload, peer=True)
        err = np.ctypeslib.as_array(C.cast(wb.result().err, C.POINTER(C.c_uint8)), shape=(count,))
        err[:] = 3
        got = wb.encode(first, count, peer=True)
        assert len(got) == n * (1 + 2 + 1 + 2 + longest)
        assert len(got) <= L.guber_wire_pool_response_bound(payload, len(payload))
        wb.close()


# what the client mode produced before the peer mode existed, for rand_reqs(default_rng(1234), 400) decoded at NOW and answered by the oracle
# (sha256 of the SoA columns and of the two encodings): the client decode and encode stay byte-identical
def _client_digest():
    import hashlib
    rng = np.random.default_rng(1234)
    wb = gw.WireBatch(4096, 1 << 18)
    o = support.Oracle(cache_size=1 << 16)
    h = hashlib.sha256()
    for rpc in range(6):
        payload = wire_replay.pb_request(rand_reqs(rng, int(rng.integers(1, 400))), peer=bool(rpc & 1))
        wb.reset(NOW + rpc)
        first, count = wb.decode(payload, max_per_rpc=1000, is_owner=not (rpc & 2))
        arr = wb.arrays()
        for k in ("hits", "limit", "duration", "burst", "created_at", "algorithm", "behavior", "is_owner"):
            h.update(arr[k].tobytes())
        h.update(b"|".join(arr["keys"])); h.update(wb.pre_errors().tobytes())
        o.lib.oracle_eval_batch(o.h, C.byref(wb.view()), C.byref(wb.result()))
        h.update(wb.encode(first, count, wrap_errors=True)); h.update(wb.encode(first, count, wrap_errors=False))
    o.close(); wb.close()
    return h.hexdigest()


def test_client_mode_is_byte_identical_to_before():
    """on rand_reqs payloads: the SoA columns, the validation codes and both encodings of the client mode hash to what they hashed to on the
    commit before the peer mode (the digest below was taken there), and equal the protobuf runtime's view as tests/test_wire_cpu.py checks"""
    assert _client_digest() == CLIENT_DIGEST_BEFORE


CLIENT_DIGEST_BEFORE = "532837489f92fe40e476a93dd7372e196d9aafaf576748ccab8e7e6d63802472"


def test_the_peer_handlers_c99_file_compiles_and_fails_loudly_without_a_device(tmp_path):
    """tests/hostsim/peer_abi_c99.c (the call sequence of go/wire_server.go's two peer handlers): plain C99 against the public headers, links
    the product library; without a GPU its engine creation fails with GUBER_E_NO_DEVICE (exit 0).  With one, tests/test_gpu_wire_peer.py runs it."""
    import torch
    if not os.path.exists(ga.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exe = str(tmp_path / "peer_abi_c99")
    libdir = os.path.join(support.ROOT, "gubernator_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(support.ROOT, "include"), "-o", exe,
                    os.path.join(support.ROOT, "tests", "hostsim", "peer_abi_c99.c"), "-L", libdir, "-lguber_hip", f"-Wl,-rpath,{libdir}"], check=True)
    if torch.cuda.is_available():
        return                                                    # (the GPU suite runs it with --gpu)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and ("no HIP device" in r.stdout or "no CPU fallback" in r.stdout), (r.returncode, r.stdout, r.stderr)


def _runtime(name):
    return subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True, check=True).stdout.strip()


def test_the_gpu_suites_peer_file_against_the_cpu_engine():
    """tests/test_gpu_wire_peer.py — the `-m gpu` tests of the peer RPCs on the payload stage — unchanged, in a process of its own, against the
    CPU build of the engine under AddressSanitizer (tests/test_enginesim_cpu.py starts the other payload-stage files the same way): k_wire_fill's
    peer branch, the stages, the callers' own evaluation and guber_wire_pool_update_peer_globals beside eight threads.  (The plain-C file links
    the product library itself and stays a GPU test.)"""
    hs = os.path.join(support.ROOT, "tests", "hostsim")
    subprocess.run(["make", "-s", "-C", hs, "enginesim_san_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(support.ROOT, "oracle")], check=True)
    san = dict(LD_PRELOAD=_runtime("libasan.so"), ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(support.ROOT, "tests", "test_gpu_wire_peer.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not plain_c"], capture_output=True, text=True, timeout=2400, cwd=support.ROOT,
                       env=dict(os.environ, GUBER_HIP_LIB=os.path.join(hs, "libenginesim_san.so"), **san))
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0 and " passed" in p.stdout and "failed" not in p.stdout, tail
