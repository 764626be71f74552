"""The key path without a GPU.  The hash: xxhash64_words4_uniform (gubernator_amd/csrc/guber_algo.h, what k_fr_count / k_part / k_front
hash a fixed-width key with) equals xxhash64 for every length 1 .. 31 on random bytes with garbage in the words behind the key, a
plain-Python XXH64 and the known answers of tests/golden/kat_vectors.json.  The pipelines: tests/key_path_cases.py's generations at
their smallest sizes on the CPU build of the engine (tests/hostsim/enginesim.cpp: host code and kernels compiled for the host), fronts
of 1, 3 and 16 engines, in a process of its own.  (That build runs plain here; the same path under AddressSanitizer is the stand-alone
program of tests/test_key_path_asan_cpu.py.)"""
import json
import os
import subprocess
import sys

import numpy as np

import front_edges as fe
from support import ROOT

HS = os.path.join(ROOT, "tests", "hostsim")


def _hashes(tmp_path, rows):
    """rows of (len, 32 bytes) -> [(xxhash64, xxhash64_words4, xxhash64_words4_uniform)]"""
    exe = str(tmp_path / "key_path_hash")
    c = subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HS, "key_path_hash.cpp")], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], input="".join(f"{n} {bytes(b).hex()}\n" for n, b in rows), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [tuple(int(x) for x in line.split()) for line in p.stdout.splitlines()]
    assert len(out) == len(rows)
    return out


def test_the_uniform_length_hash_is_xxh64_for_every_length_below_32(tmp_path):
    rng = np.random.default_rng(64)
    rows = [(n, rng.integers(0, 256, 32, dtype=np.uint8)) for n in range(1, 32) for _ in range(8)]
    for n in range(1, 32):                                            # (and with all bits set behind the key)
        b = rng.integers(0, 256, 32, dtype=np.uint8); b[n:] = 0xFF
        rows.append((n, b))
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_vectors.json")))["xxh64"]
    pattern = bytes((37 * i + 11) % 251 + 1 for i in range(64))       # (the file's pattern: byte i = (37 i + 11) mod 251 + 1)
    known = {v["len"]: v["xxh64"] for v in kat["vectors"] if v["seed"] == 0 and 1 <= v["len"] <= 31}
    for n in known:
        b = np.frombuffer(pattern[:32], np.uint8).copy(); b[n:] ^= 0x5A
        rows.append((n, b))
    got = _hashes(tmp_path, rows)
    for (n, b), (h, h4, hu) in zip(rows, got):
        assert h == h4 == hu == fe.xxh64(bytes(b[:n])), (n, bytes(b).hex(), h, h4, hu)
    checked = 0
    for (n, b), (h, h4, hu) in zip(rows[-len(known):], got[-len(known):]):
        assert hu == known[n], (n, hu, known[n])
        checked += 1
    assert checked == len(known)                                      # (every length 1 .. 31 the file has: 1, 8, 16 and 31 where they are there)
    print("known answers checked for the lengths", sorted(known))


def test_fixed_width_shares_through_every_pipeline_on_the_cpu_engine():
    subprocess.run(["make", "-s", "-C", HS, "enginesim_lib"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "key_path_cases.py")], capture_output=True, text=True, timeout=1500,
                       env=dict(os.environ, GUBER_HIP_LIB=os.path.join(HS, "libenginesim.so")))
    assert p.returncode == 0 and "KEY PATH CASE OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
