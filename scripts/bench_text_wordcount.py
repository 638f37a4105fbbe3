#!/usr/bin/env python3
"""Secondary measurement (not the driver bench line): word count over raw
text bytes with the device tokenizer and string hasher.

--stages  device stage rates at 1 GiB of text: tokenize, hash, build,
          lookup, first-token, each timed with device events (2 warm-ups,
          5 repetitions, minimum and spread reported), as GB/s of text and
          as a share of the HBM bound from the bytes model below.
--e2e     end to end at 64 MiB: examples/word_count/word_count FILE (the
          host tokenize+hash path) against word_count --device-text FILE,
          wall clock around each child process, 3 alternating runs each;
          the two outputs must be identical files.

The text comes from a seed: Zipf(1.1) ids over a 1M vocabulary, each id
spelled as a deterministic lowercase word (base 26 of id+26: 2-5 letters,
frequent words are short), single spaces, a newline every 16 words, cut at
the byte target. Results are merged into the --out JSON.

Bytes model (per stage, N text bytes, T tokens, M distinct words, C table
slots) — the least HBM traffic the stage's algorithm needs:
  tokenize     2N (count pass + scatter pass) + 8T (off, len written)
  hash         N + 8T (off, len read) + 16T (k1, k2 written)
  build        16T (k1, k2 read) + 48M (each used slot read and written)
  lookup       16T read + 4T written + 24M (each used slot read once)
  first_token  4T read + 4C (first[] initialised) + 4M
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12       # B/s, MI355X HBM3E specification peak
VOCAB = 1_000_000
ZIPF_S = 1.1
SEED = 0x7E87
CHUNK_TOKENS = 1 << 22  # a multiple of 16, so newlines line up per chunk
W = 6                   # longest spelling (5 letters) + its delimiter


def vocabulary():
    """[VOCAB, W] byte matrix of spellings (0 = unused) and their lengths"""
    ids = np.arange(VOCAB, dtype=np.int64) + 26
    mat = np.zeros((VOCAB, W), np.uint8)
    ndig = np.ones(VOCAB, np.int64)
    for k in range(1, 6):
        ndig[ids >= 26 ** k] = k + 1
    for pos in range(5):            # most significant letter first
        p = ndig - 1 - pos
        ok = p >= 0
        mat[ok, pos] = (ids[ok] // 26 ** p[ok]) % 26 + ord("a")
    return mat, ndig


def zipf_cdf():
    w = 1.0 / np.arange(1, VOCAB + 1, dtype=np.float64) ** ZIPF_S
    c = np.cumsum(w)
    return c / c[-1]


def make_chunk(args):
    c, cdf, mat, ndig = args
    rng = np.random.default_rng([SEED, c])
    ids = np.searchsorted(cdf, rng.random(CHUNK_TOKENS)).clip(0, VOCAB - 1)
    rows = mat[ids]
    delim = np.full(CHUNK_TOKENS, 0x20, np.uint8)
    delim[15::16] = 0x0A
    rows[np.arange(CHUNK_TOKENS), ndig[ids]] = delim
    return rows[rows != 0].tobytes()


def make_text(nbytes):
    cdf = zipf_cdf()
    mat, ndig = vocabulary()
    parts, have, c = [], 0, 0
    with ThreadPoolExecutor(16) as pool:
        while have < nbytes:
            batch = list(pool.map(make_chunk, [(c + i, cdf, mat, ndig)
                                               for i in range(16)]))
            for b in batch:
                if have < nbytes:
                    parts.append(b)
                    have += len(b)
            c += 16
    return b"".join(parts)[:nbytes]


def stages(nbytes, reps=5, warm=2):
    import torch
    from thrill_amd import Native, T9Error
    from thrill_amd.pipeline import _ptr, _stream
    t0 = time.perf_counter()
    data = make_text(nbytes)
    print(f"# generated {len(data)} bytes in {time.perf_counter() - t0:.1f}"
          " s", file=sys.stderr)
    nat, s = Native(device=0), _stream()
    i32, i64 = torch.int32, torch.int64
    d_text = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    del data
    d_n = torch.empty(1, dtype=i64, device="cuda")
    d_err = torch.empty(1, dtype=i32, device="cuda")
    d_ws = torch.empty(int(nat.ws("text_tokenize", nbytes)),
                       dtype=torch.uint8, device="cuda")
    nat.text_tokenize(_ptr(d_text), nbytes, None, None, _ptr(d_n),
                      _ptr(d_ws), s)
    T = int(d_n.cpu().item())
    d_off = torch.empty(T, dtype=i32, device="cuda")
    d_len = torch.empty(T, dtype=i32, device="cuda")
    d_k1 = torch.empty(T, dtype=i64, device="cuda")
    d_k2 = torch.empty(T, dtype=i64, device="cuda")
    d_slot = torch.empty(T, dtype=i32, device="cuda")
    C = 1 << max(10, (2 * T + 1).bit_length())   # TextWordCount's default
    d_tbl = torch.empty(nat.reduce128_table_words(C), dtype=i64,
                        device="cuda")
    d_first = torch.empty(C, dtype=i32, device="cuda")

    def timed(name, fn, before=None):
        ms = []
        for r in range(warm + reps):
            if before:
                before()
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warm:
                ms.append(a.elapsed_time(b))
        print(f"# {name}: {['%.3f' % m for m in ms]} ms", file=sys.stderr)
        return ms

    t = {}
    t["tokenize"] = timed("tokenize", lambda: nat.text_tokenize(
        _ptr(d_text), nbytes, _ptr(d_off), _ptr(d_len), _ptr(d_n),
        _ptr(d_ws), s))
    assert int(d_n.cpu().item()) == T
    t["hash"] = timed("hash", lambda: nat.text_hash2(
        _ptr(d_text), nbytes, _ptr(d_off), _ptr(d_len), T, _ptr(d_k1),
        _ptr(d_k2), _ptr(d_err), s))
    assert int(d_err.cpu().item()) == 0
    t["build"] = timed(
        "build",
        lambda: nat.reduce128_build(_ptr(d_k1), _ptr(d_k2), None, T,
                                    _ptr(d_tbl), C, 0, _ptr(d_err), s),
        before=lambda: nat.reduce128_init(_ptr(d_tbl), C, s))
    if int(d_err.cpu().item()):
        raise T9Error("table overflow")
    t["lookup"] = timed("lookup", lambda: nat.reduce128_lookup(
        _ptr(d_k1), _ptr(d_k2), T, _ptr(d_tbl), C, 0, _ptr(d_slot), s))
    t["first_token"] = timed("first_token", lambda: nat.text_first_token(
        _ptr(d_slot), T, _ptr(d_first), C, s))
    # the stages computed a word count: every token landed in a group
    assert int((d_slot < 0).sum().item()) == 0
    M = int((d_first != -1).sum().item())
    counts = d_tbl.view(C, 3)[:, 2]
    assert int(counts.sum().item()) == T
    nat.close()

    N = nbytes
    model = {
        "tokenize": 2 * N + 8 * T,
        "hash": N + 8 * T + 16 * T,
        "build": 16 * T + 48 * M,
        "lookup": 16 * T + 4 * T + 24 * M,
        "first_token": 4 * T + 4 * C + 4 * M,
    }
    out = {}
    for k, ms in t.items():
        best = min(ms)
        out[k] = {
            "min_ms": round(best, 3),
            "max_ms": round(max(ms), 3),
            "spread_pct": round(100 * (max(ms) - best) / best, 1),
            "text_GBps": round(N / (best * 1e-3) / 1e9, 1),
            "model_bytes": model[k],
            "model_GBps": round(model[k] / (best * 1e-3) / 1e9, 1),
            "share_of_hbm_bound_pct": round(
                100 * (model[k] / HBM_PEAK) / (best * 1e-3), 1),
        }
    worst = min(out, key=lambda k: out[k]["share_of_hbm_bound_pct"])
    return {
        "text_bytes": N, "tokens": T, "distinct_words": M,
        "table_slots": C, "reps": reps, "warmups": warm,
        "hbm_peak_Bps": HBM_PEAK, "timing": "device events",
        "stages": out, "furthest_from_bound": worst,
        "sum_of_stage_min_ms": round(sum(v["min_ms"] for v in out.values()),
                                     3),
    }


def e2e(nbytes, runs=3, host_limit=600, dev_limit=300):
    exe = os.path.join(REPO, "examples", "word_count", "word_count")
    if not os.path.exists(exe):
        raise SystemExit(f"{exe} not built (python __graft_entry__.py)")
    res = {"text_bytes": nbytes, "runs": runs, "timing":
           "wall clock around each child process", "host_s": [],
           "device_text_s": []}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "text.in")
        with open(src, "wb") as f:
            f.write(make_text(nbytes))
        outs = {"host": os.path.join(tmp, "host.out"),
                "device_text": os.path.join(tmp, "dev.out")}
        cmds = {"host": ([exe, src, outs["host"]], host_limit),
                "device_text": ([exe, "--device-text", src,
                                 outs["device_text"]], dev_limit)}
        for r in range(runs):
            for which in ("host", "device_text"):
                cmd, limit = cmds[which]
                t0 = time.perf_counter()
                try:
                    p = subprocess.run(cmd, timeout=limit,
                                       capture_output=True, text=True)
                except subprocess.TimeoutExpired:
                    # recorded as the result; nothing more is started
                    res[which + "_timeout_s"] = limit
                    return res
                dt = time.perf_counter() - t0
                if p.returncode != 0:
                    res[which + "_failed"] = {"rc": p.returncode,
                                              "stderr": p.stderr[-500:]}
                    return res
                res[which + "_s"].append(round(dt, 3))
                print(f"# run {r} {which}: {dt:.3f} s", file=sys.stderr)
        with open(outs["host"], "rb") as a, \
                open(outs["device_text"], "rb") as b:
            ha, hb = a.read(), b.read()
        res["output_bytes"] = len(ha)
        res["outputs_identical"] = ha == hb
    res["ratio_fastest_host_over_slowest_device_text"] = round(
        min(res["host_s"]) / max(res["device_text_s"]), 2)
    res["device_text_always_faster"] = \
        max(res["device_text_s"]) < min(res["host_s"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--stage-bytes", type=int, default=1 << 30)
    ap.add_argument("--e2e-bytes", type=int, default=64 << 20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "text_wordcount.json"))
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.setdefault("metric", "word count over raw text bytes, 1 GPU")
    res.setdefault("generator", f"zipf({ZIPF_S}) ids over {VOCAB} words, "
                   f"seed {SEED:#x}, base-26 spellings, newline every 16")
    if a.stages:
        res["device_stages"] = stages(a.stage_bytes)
    if a.e2e:
        res["end_to_end"] = e2e(a.e2e_bytes)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    e = res.get("end_to_end", {})
    if a.e2e and not (e.get("outputs_identical")
                      and e.get("device_text_always_faster")):
        raise SystemExit("end-to-end requirement not met")


if __name__ == "__main__":
    main()
