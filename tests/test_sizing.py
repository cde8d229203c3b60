"""The sizing rules of a clustering call (hammock_amd/csrc/hmk_sizing.h) against the formulas the host code had in several copies
before they were written once: band request, adjacency entry format, first edge-buffer capacity, capacity after an overflow.
Host-only code: tests/tools/sizing_probe.cpp is compiled with the host C++ compiler and fed the table below."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARDS = 64   # HMK_EDGE_SHARDS (the probe prints the header's value first)


# ---- the earlier formulas, literally ------------------------------------------------------------------------------------------
def old_band(n, max_clusters):
    """hmk_greedy_cluster / greedy_cluster_multi (without their HMK_NO_BAND / clinkage conditions) and hmk_reserve."""
    band = 0
    if max_clusters > 0 and n >= 16384:
        band = min(n, 2 * max_clusters + 1024)
    if band * 2 > n:
        band = 0
    return band


def old_packed(max_len, min_len, max_m, shift_penalty, max_shift, threshold, force_8byte):
    top = max_len * max(0, max_m) + max(0, shift_penalty) * ((max_len - min_len) + 2 * max_shift)
    return int(top - threshold <= 255 and not force_8byte)


def old_guess(symmetric, n, devices, forced, have):
    k = 0.003 if symmetric else 0.006
    if devices == 1:    # first_edge_capacity
        guess = int(float(n) * (n - 1) / 2 * k) + (1 << 20)
    else:               # greedy_cluster_multi (`have` = the larger of the device's buffer and what an overflow asked for)
        guess = int(float(n) * (n - 1) / 2 * k / devices * 1.25) + (1 << 20)
    if forced:
        guess = forced
    cap = max(min(guess, 1 << 31), 1 << 20, have)
    return (cap + SHARDS - 1) // SHARDS * SHARDS


def old_overflow(mx):
    return SHARDS * (mx + mx // 8 + 1024)


def default_max_clusters(n):   # hmk_reserve: Hammock.java's default cluster limit
    return int(n * 0.025 + 0.5)


def table():
    rows = []
    # band: both sides of n = 16384; no cluster limit; the default limit, down to where its band first exceeds n / 2 (far below
    # 16384: the default never loses its band to that rule); limits that put the band exactly at n / 2 and just above
    exceeds = [n for n in range(2, 20000) if 2 * min(n, 2 * default_max_clusters(n) + 1024) > n]
    n_half = max(exceeds)
    assert n_half == 2275
    for n in (2, 16383, 16384, n_half, n_half + 1, 10 ** 5, 10 ** 6, 2 ** 24):
        for maxc in (0, -1, 1, default_max_clusters(n)):
            rows.append(("band", n, maxc))
    rows += [("band", 16384, 3584), ("band", 16384, 3585), ("band", 16384, 10 ** 6), ("band", 10 ** 5, 24488), ("band", 10 ** 5, 24489),
             ("band", 10 ** 6, 2 ** 31 - 1)]
    # packed: top - threshold exactly 255 and 256, with and without a shift penalty, unequal lengths, negative matrix maximum,
    # negative threshold, the force switch
    for force in (0, 1):
        rows += [("packed", 12, 12, 11, 0, 3, 12 * 11 - 255, force), ("packed", 12, 12, 11, 0, 3, 12 * 11 - 256, force),
                 ("packed", 20, 7, 17, 2, 3, 20 * 17 + 2 * (13 + 6) - 255, force), ("packed", 20, 7, 17, 2, 3, 20 * 17 + 2 * (13 + 6) - 256, force),
                 ("packed", 20, 7, 17, -4, 3, 20 * 17 - 255, force), ("packed", 20, 7, 17, -4, 3, 20 * 17 - 256, force),
                 ("packed", 32, 1, -3, 5, 0, 5 * 31 - 255, force), ("packed", 32, 1, -3, 5, 0, 5 * 31 - 256, force),
                 ("packed", 32, 32, 1000, 1000, 31, 0, force), ("packed", 12, 12, 11, 0, 0, -124, force), ("packed", 12, 12, 11, 0, 0, -123, force)]
    # guess: one, two and eight devices; tiny to 10^6 (asymmetric 10^6 on one device: a guess above 2^31); forced guesses; `have`
    # below, at and above the guess
    for sym in (1, 0):
        for n in (2, 3000, 10 ** 5, 10 ** 6, 2 ** 24):
            for dev in (1, 2, 8):
                for forced in (0, 1, 2 ** 33):
                    g = old_guess(sym, n, dev, forced, 0)
                    for have in (0, 1, g - SHARDS, g, g + 1, g + SHARDS, 2 ** 32 + 5):
                        rows.append(("guess", sym, n, dev, forced, max(have, 0)))
    rows += [("overflow", v) for v in (0, 1, 7, 8, 2 ** 20, 2 ** 31, 2 ** 40)]
    return rows


OLD = {"band": old_band, "packed": old_packed, "guess": old_guess, "overflow": old_overflow}


def test_sizing_rules_equal_the_formulas_they_replace(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    probe = str(tmp_path / "sizing_probe")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-o", probe,
                           os.path.join(ROOT, "tests", "tools", "sizing_probe.cpp")])
    rows = table()
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    out = subprocess.run([probe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0] == f"shards = {SHARDS}"
    assert len(out) == 1 + len(rows)
    bad = []
    for r, line in zip(rows, out[1:]):
        asked, got = line.split(" = ")
        assert asked == " ".join(str(v) for v in r)
        want = OLD[r[0]](*r[1:])
        if int(got) != want:
            bad.append((line, want))
    assert not bad, bad[:10]
    # the table holds what it is meant to: both answers of every rule, a guess above 2^31, both sides of the half-n rule
    assert {old_packed(*r[1:]) for r in rows if r[0] == "packed"} == {0, 1}
    assert any(r[0] == "band" and r[1] >= 16384 and r[2] > 0 and old_band(*r[1:]) == 0 for r in rows)
    assert any(r[0] == "band" and old_band(*r[1:]) > 0 for r in rows)
    assert ("guess", 0, 10 ** 6, 1, 0, 0) in rows and old_guess(0, 10 ** 6, 1, 0, 0) == 2 ** 31 < int(float(10 ** 6) * (10 ** 6 - 1) / 2 * 0.006)
