"""Real text on the device: tokenizer, string hasher, table lookup,
first-token pick, and the word count built from them.

The tokenizer's contract is the reference pipeline's split — ReadLines at
'\\n' (thrill/api/read_lines.hpp), WordCount at ' ' dropping empty words
(examples/word_count/word_count.hpp:37-45) — so the host model is
re.finditer(rb'[^ \\n]+'): offsets, lengths and count must match exactly.
The hasher must be bit-equal to detail::string_hash2 (include/t9/dia.hpp),
restated here in pure Python with the oracle's Hash128to64.

The `~0 -> ^= 1` sentinel remap of the hasher cannot be reached from a
test: that would take a preimage of ~0 under FNV-1a + Hash128to64. That
branch is covered by reading the code only (it is the same two lines as
string_hash2's and t9_hash2_of's).
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G
    from thrill_amd import Native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TOKEN = re.compile(rb"[^ \n]+")
ABSENT = 0xFFFFFFFF
T9_EINVAL = -22


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


def random_text(n, seed):
    """' ' with probability 1/6, '\\n' 1/40, the rest uniform over every
    other byte value (0x00, '\\t', '\\r' and 0x80-0xFF included)."""
    rng = np.random.default_rng(seed)
    words = np.array([b for b in range(256) if b not in (0x20, 0x0A)],
                     dtype=np.uint8)
    out = words[rng.integers(0, len(words), n)]
    u = rng.random(n)
    out[u < 1 / 6] = 0x20
    out[(u >= 1 / 6) & (u < 1 / 6 + 1 / 40)] = 0x0A
    return out.tobytes()


@pytest.fixture(scope="module")
def rand_buf():
    return random_text((1 << 20) + 3, seed=0x7E47)


def dev_text(data):
    return G.dev(np.frombuffer(data, dtype=np.uint8).copy())


def tokenize(nat, data, count_only=False):
    n = len(data)
    d_text = dev_text(data)
    cap = max((n + 1) // 2, 1)
    d_n = G.dev(np.array([12345], np.uint64))   # must be overwritten
    w = G.ws(nat.ws("text_tokenize", n))
    if count_only:
        nat.text_tokenize(G.ptr(d_text), n, None, None, G.ptr(d_n),
                          G.ptr(w), G.stream())
        return int(G.host(d_n, np.uint64)[0])
    d_off, d_len = G.empty(cap, np.uint32), G.empty(cap, np.uint32)
    nat.text_tokenize(G.ptr(d_text), n, G.ptr(d_off), G.ptr(d_len),
                      G.ptr(d_n), G.ptr(w), G.stream())
    m = int(G.host(d_n, np.uint64)[0])
    assert m <= cap
    return (G.host(d_off, np.uint32)[:m].copy(),
            G.host(d_len, np.uint32)[:m].copy(), m)


def check_tokens(nat, data):
    exp = [(t.start(), t.end() - t.start()) for t in TOKEN.finditer(data)]
    off, ln, m = tokenize(nat, data)
    print(f"nbytes={len(data)} tokens: got {m} expected {len(exp)}")
    assert m == len(exp)
    assert np.array_equal(off, np.array([e[0] for e in exp], np.uint32))
    assert np.array_equal(ln, np.array([e[1] for e in exp], np.uint32))
    assert tokenize(nat, data, count_only=True) == len(exp)


SMALL = {
    "empty": b"",
    "one_word_byte": b"x",
    "one_space": b" ",
    "one_newline": b"\n",
    "15": b"ab cd\nef  gh\nij",
    "16": b"ab cd\nef  gh\nijk",
    "17": b"ab cd\nef  gh\nijk ",
    "17_straddle": b"0123456789abcdefg",
    "16_then_word": b"               x",
    "all_spaces": b" " * 5000,
    "all_newlines": b"\n" * 4099,
    "lead_trail": b" \n  lead and trail \n\n ",
    "runs_1_to_5": b"a b  c\n\n\nd \n \ne\n \n \nf",
    "other_bytes": b"\x00 \t\r\n\x80\xff \x00\x00\n\x1f!\x0b",
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_tokenize_small(nat, name):
    check_tokens(nat, SMALL[name])


def test_tokenize_no_delimiter(nat):
    """one token of 1<<18 bytes: several tiles, no start or stop inside"""
    check_tokens(nat, b"w" * (1 << 18))
    check_tokens(nat, b" " + b"w" * (1 << 18))


def test_tokenize_random(nat, rand_buf):
    check_tokens(nat, rand_buf)


def test_tokenize_long_run_spliced(nat, rand_buf):
    """a 300 000-byte delimiter-free run in the middle: one token spans
    many tiles, ordinary tokens on both sides"""
    mid = len(rand_buf) // 2
    check_tokens(nat, rand_buf[:mid] + b"\xc3" * 300_000 + rand_buf[mid:])


def test_tokenize_rejects_4gib(nat):
    d_text = dev_text(b"tiny")
    d_n = G.empty(1, np.uint64)
    w = G.ws(256)
    for nbytes in (1 << 32, (1 << 32) + 5, 1 << 40):
        rc = nat._lib.t9_text_tokenize(nat.ctx, G.ptr(d_text), nbytes, None,
                                       None, G.ptr(d_n), G.ptr(w),
                                       G.stream())
        assert rc == T9_EINVAL


# ---------------------------------------------------------------- hasher

def fnv1a(data, basis):
    h = basis
    for b in data:
        h = ((h ^ b) * 0x100000001B3) % (1 << 64)
    return h


def host_hash2(oracle, word):
    h1 = oracle.hash128to64(0x9AE16A3B2F90404F,
                            fnv1a(word, 0xCBF29CE484222325))
    h2 = oracle.hash128to64(0xC3A5C85C97CB3127,
                            fnv1a(word, 0x84222325CBF29CE4))
    if h1 == 2**64 - 1:
        h1 ^= 1
    if h2 == 2**64 - 1:
        h2 ^= 1
    return h1, h2


def dev_hash2(nat, data, offs, lens):
    n = len(offs)
    d_text = dev_text(data)
    d_off = G.dev(np.asarray(offs, np.uint32))
    d_len = G.dev(np.asarray(lens, np.uint32))
    d_k1, d_k2 = G.empty(max(n, 1), np.uint64), G.empty(max(n, 1), np.uint64)
    d_err = G.dev(np.array([77], np.uint32))   # must be zeroed by the call
    nat.text_hash2(G.ptr(d_text), len(data), G.ptr(d_off), G.ptr(d_len), n,
                   G.ptr(d_k1), G.ptr(d_k2), G.ptr(d_err), G.stream())
    return (G.host(d_k1, np.uint64)[:n], G.host(d_k2, np.uint64)[:n],
            int(G.host(d_err, np.uint32)[0]))


def check_hashes(nat, oracle, data, ranges):
    offs = [r[0] for r in ranges]
    lens = [r[1] for r in ranges]
    k1, k2, err = dev_hash2(nat, data, offs, lens)
    assert err == 0
    cache = {}
    for i, (o, l) in enumerate(ranges):
        w = data[o:o + l]
        if w not in cache:
            cache[w] = host_hash2(oracle, w)
        assert (int(k1[i]), int(k2[i])) == cache[w], (i, o, l)


def test_hash2_random_tokens(nat, oracle, rand_buf):
    data = rand_buf[12345:12345 + (64 << 10)]
    ranges = [(t.start(), t.end() - t.start())
              for t in TOKEN.finditer(data)]
    assert len(ranges) > 5000
    check_hashes(nat, oracle, data, ranges)


def test_hash2_handmade_ranges(nat, oracle, rand_buf):
    data = rand_buf[:80_000]
    n = len(data)
    ranges = [(0, 0), (5, 0), (n, 0)]                     # empty string
    ranges += [(o, l) for o in range(40, 48) for l in range(1, 18)]
    ranges += [(3, 70_000)]                               # one long chain
    ranges += [(n - 1, 1), (n - 5, 5), (n - 13, 13), (0, n)]   # last byte
    ranges += [(100, 30), (110, 30), (100, 30)]           # overlapping
    check_hashes(nat, oracle, data, ranges)
    # a buffer whose length is no multiple of 8: the last partial word
    odd = rand_buf[:1003]
    check_hashes(nat, oracle, odd,
                 [(1003 - l, l) for l in range(0, 20)] + [(0, 1003)])


def test_hash2_out_of_range_is_reported_not_read(nat, oracle):
    """ordinary argument validation: the kernel compares off+len with
    nbytes BEFORE any load, so nothing is read and nothing faults"""
    data = b"alpha beta gamma"
    n = len(data)
    ranges = [(0, 5), (n - 2, 3), (6, 4), (n + 7, 1), (0xFFFFFFFF, 0xFFFFFFFF)]
    k1, k2, err = dev_hash2(nat, data, [r[0] for r in ranges],
                            [r[1] for r in ranges])
    assert err != 0
    for i in (0, 2):   # the valid entries are still hashed
        o, l = ranges[i]
        assert (int(k1[i]), int(k2[i])) == host_hash2(oracle, data[o:o + l])
    # and a fully valid call clears the flag again
    assert dev_hash2(nat, data, [0], [n])[2] == 0


# ---------------------------------------------------------------- lookup

def build_table(nat, k1, k2, cap):
    d1, d2 = G.dev(k1), G.dev(k2)
    tbl = G.empty(3 * cap, np.uint64)
    derr, dn = G.empty(1, np.uint32), G.empty(1, np.uint64)
    o1, o2, ov = (G.empty(cap, np.uint64) for _ in range(3))
    s = G.stream()
    nat.reduce128_init(G.ptr(tbl), cap, s)
    nat.reduce128_build(G.ptr(d1), G.ptr(d2), None, len(k1), G.ptr(tbl), cap,
                        0, G.ptr(derr), s)
    nat.reduce128_drain(G.ptr(tbl), cap, G.ptr(o1), G.ptr(o2), G.ptr(ov),
                        G.ptr(dn), s)
    assert int(G.host(derr, np.uint32)[0]) == 0
    return tbl, int(G.host(dn, np.uint64)[0])


def lookup(nat, tbl, cap, k1, k2):
    d_slot = G.empty(len(k1), np.uint32)
    d1, d2 = G.dev(k1), G.dev(k2)
    nat.reduce128_lookup(G.ptr(d1), G.ptr(d2), len(k1), G.ptr(tbl), cap, 0,
                         G.ptr(d_slot), G.stream())
    return G.host(d_slot, np.uint32)


def test_lookup_present_absent(nat):
    rng = np.random.default_rng(5)
    cap = 1 << 10
    keys = rng.integers(1, 2**63, size=(300, 2), dtype=np.uint64)
    keys[:8, 0] = keys[0, 0]          # 8 keys share k1, differ in k2
    assert len({tuple(k) for k in keys.tolist()}) == 300
    pick = rng.integers(0, 300, 5000)
    pick[:300] = np.arange(300)       # every key at least once
    k1 = np.ascontiguousarray(keys[pick, 0])
    k2 = np.ascontiguousarray(keys[pick, 1])
    tbl, m = build_table(nat, k1, k2, cap)
    assert m == 300
    slots = lookup(nat, tbl, cap, k1, k2)
    assert (slots < cap).all()
    by_key = {}
    for p, s in zip(pick.tolist(), slots.tolist()):
        assert by_key.setdefault(p, s) == s           # equal keys, one slot
    assert len(set(by_key.values())) == 300           # distinct keys differ

    absent = rng.integers(1, 2**63, size=(100, 2), dtype=np.uint64)
    absent[0, 0] = keys[0, 0]         # present k1 (a probed chain), absent k2
    absent[1, 0] = keys[50, 0]
    present = {tuple(k) for k in keys.tolist()}
    assert not any(tuple(a) in present for a in absent.tolist())
    got = lookup(nat, tbl, cap, np.ascontiguousarray(absent[:, 0]),
                 np.ascontiguousarray(absent[:, 1]))
    assert (got == ABSENT).all()


def test_lookup_full_table_terminates(nat):
    """no empty slot to stop at: only the capacity bound ends the probe"""
    rng = np.random.default_rng(6)
    cap = 1 << 10
    keys = rng.integers(1, 2**63, size=(cap, 2), dtype=np.uint64)
    assert len({tuple(k) for k in keys.tolist()}) == cap
    k1 = np.ascontiguousarray(keys[:, 0])
    k2 = np.ascontiguousarray(keys[:, 1])
    tbl, m = build_table(nat, k1, k2, cap)
    assert m == cap
    slots = lookup(nat, tbl, cap, k1, k2)
    assert sorted(slots.tolist()) == list(range(cap))
    miss = np.array([0x1234567], np.uint64)
    assert lookup(nat, tbl, cap, miss, miss)[0] == ABSENT


def test_first_token(nat):
    rng = np.random.default_rng(7)
    cap, n = 1 << 10, 1 << 18
    used = rng.permutation(cap)[:cap - 50].astype(np.uint32)   # 50 untouched
    slot = used[rng.integers(0, len(used), n)]
    slot[rng.random(n) < 0.05] = ABSENT
    slot[:7] = ABSENT
    exp = np.full(cap, ABSENT, np.uint32)
    ok = slot != ABSENT
    np.minimum.at(exp, slot[ok], np.arange(n, dtype=np.uint32)[ok])
    d_first = G.dev(np.zeros(cap, np.uint32))     # initialised by the call
    d_slot = G.dev(slot)
    nat.text_first_token(G.ptr(d_slot), n, G.ptr(d_first), cap, G.stream())
    got = G.host(d_first, np.uint32)
    assert (exp == ABSENT).sum() >= 50
    assert np.array_equal(got, exp)


# ------------------------------------------------------------ word count

def test_text_wordcount_bacon_ipsum_kat():
    from thrill_amd.pipeline import TextWordCount
    with open(os.path.join(GOLDEN, "wordcount.in"), "rb") as f:
        data = f.read()
    with open(os.path.join(GOLDEN, "bacon_ipsum_correct.json")) as f:
        table = json.load(f)
    wc = TextWordCount()
    try:
        got = wc.count(data)
        assert wc.count(b"") == {} and wc.count(b" \n \n") == {}
    finally:
        wc.close()
    assert {w.decode(): c for w, c in got.items()} == table


def test_text_wordcount_first_occurrence():
    """each group's (offset, length) names the word's FIRST occurrence:
    a 7-letter alphabet makes most words repeat many times"""
    from thrill_amd.pipeline import TextWordCount
    rng = np.random.default_rng(8)
    data = rng.choice(np.frombuffer(b"abcde \n", np.uint8), 200_003,
                      p=[.17, .17, .17, .17, .12, .17, .03]).tobytes()
    first, counts = {}, {}
    for t in TOKEN.finditer(data):
        first.setdefault(t.group(), t.start())
        counts[t.group()] = counts.get(t.group(), 0) + 1
    assert max(counts.values()) > 500 and len(counts) > 1024
    wc = TextWordCount()
    try:
        offs, lens, cnts = wc.groups(data)
        assert wc.count(data) == counts
        # more distinct words than slots: the overflow flag raises
        from thrill_amd import T9Error
        with pytest.raises(T9Error):
            wc.count(data, capacity=1024)
    finally:
        wc.close()
    assert len(offs) == len(counts)
    for o, l, c in zip(offs.tolist(), lens.tolist(), cnts.tolist()):
        w = data[o:o + l]
        assert first[w] == o, (w, o, first[w])
        assert counts[w] == c


def test_word_count_example_device_text(tmp_path):
    exe = os.path.join(REPO, "examples", "word_count", "word_count")
    assert os.path.exists(exe), f"{exe} not built (__graft_entry__.build)"
    src = os.path.join(GOLDEN, "wordcount.in")
    out = str(tmp_path / "counts.txt")
    r = subprocess.run([exe, "--device-text", src, out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLDEN, "bacon_ipsum_correct.json")) as f:
        table = json.load(f)
    got = {}
    for line in open(out):
        line = line.rstrip("\n")
        if not line:
            continue
        w, c = line.rsplit(": ", 1)
        got[w] = int(c)
    assert len(got) == 71
    assert got == table
