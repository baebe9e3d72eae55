"""csrc/kernels/xgmi_plan.h (the slice rule and the bucket and shard planners behind PeerExchange
and AsyncPeer) as a stand-alone host program, csrc/kernels/tests/xgmi_plan_check.cpp, built with
AddressSanitizer + UndefinedBehaviorSanitizer and run directly: no GPU, nothing loaded into Python.

The program is held against the twin the GPU exchange tests already trust,
tests/exchange_reference.py (equal_slices, async_slices, owner_slices, bucket_regions), on every
row of the tables of docs/DESIGN.md "The exchange kernels alone", on a sweep of sizes, on the inbox
offsets of a mixed plan, and on each refusal of the planners by its message.
"""
import os
import shutil
import subprocess

import pytest

from exchange_reference import async_slices, bucket_regions, equal_slices, owner_slices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "distributed-deep-learning_amd", "csrc", "kernels", "tests",
                   "xgmi_plan_check.cpp")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("xgmi_plan") / "xgmi_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def _run(exe, stdin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=stdin, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def _sync(total, world, rank, max_slices, repl, buckets):
    """buckets: ("equal", lo, hi) or ("owner", [(lo, hi)], state_offs, owner)."""
    text = "sync %d %d %d %d %d %d\n" % (total, world, rank, max_slices, repl, len(buckets))
    for b in buckets:
        if b[0] == "owner":
            _, runs, soffs, owner = b
            text += "%d %d " % (owner, len(runs))
            text += " ".join("%d %d %d" % (lo, hi, so) for (lo, hi), so in zip(runs, soffs)) + "\n"
        else:
            text += "-1 1 %d %d\n" % (b[1], b[2])
    return text


def _async(total, world, rank, max_slices, ranges, hosts):
    return ("async %d %d %d %d %d %d\n" % (total, world, rank, max_slices, len(ranges), len(hosts))
            + "".join("%d %d\n" % r for r in ranges) + " ".join(map(str, hosts)) + "\n")


def _cut(n, slice_, nslice):
    """Float4 counts of the slices the kernels' geometry gives (xgmi_dev.h xg_slice)."""
    got = [(min(n, s + slice_) - s) // 4 for s in range(0, n, slice_)]
    assert len(got) == nslice and slice_ % 4 == 0
    return got


def _parse_sync(rows):
    """[{bucket fields, runs: [...], end}], final row, inbox."""
    out, it = [], iter(rows)
    for r in it:
        if r[0] == "bucket":
            keys = ("owner", "lo", "c", "inbox_off", "slice", "rslot", "nslice", "nruns")
            out.append(dict(zip(keys, map(int, r[2:])), runs=[], end=None))
        elif r[0] == "run":
            out[-1]["runs"].append(tuple(map(int, r[1:])))
        elif r[0] == "end":
            out[-1]["end"] = int(r[1])
        elif r[0] == "final":
            assert r[1] == "same", r
            final = [tuple(map(int, x.split(":"))) for x in r[2:]]
        elif r[0] == "inbox":
            return out, final, int(r[1])
        else:
            raise AssertionError(r)
    raise AssertionError("no inbox row")


# docs/DESIGN.md "The exchange kernels alone": chunk, max_slices, slices in float4
CHUNKS = [(4, 128, [1]), (1020, 128, [255]), (1024, 128, [256]), (1028, 128, [129, 128]),
          (3076, 128, [193, 193, 193, 190]), (4100, 1, [1025]), (4100, 2, [513, 512]),
          (7172, 128, [225] * 7 + [218])]
# runs, max_slices, slices in float4, first slice of each run and the total
RUN_SETS = [([4], 128, [1], [0, 1]),
            ([4] * 8, 128, [1] * 8, list(range(9))),
            ([1028, 4, 2052], 128, [193, 64, 1, 193, 193, 127], [0, 2, 3, 6]),
            ([3000, 100, 1500, 8], 128, [231, 231, 231, 57, 25, 231, 144, 2], [0, 4, 5, 7, 8]),
            ([2052, 1028], 2, [385, 128, 257], [0, 2, 3]),
            ([5000, 40], 1, [630, 620, 10], [0, 2, 3])]
# shard sizes, max_slices, slices per shard
SHARD_SETS = [([4, 2044, 2052, 4100], 512, [1, 1, 2, 3]), ([4100, 4], 1, [1, 1]),
              ([6148, 2052], 2, [2, 2])]


def test_design_tables(check_exe):
    for c, ms, want in CHUNKS:
        assert equal_slices(c, ms) == want  # the twin agrees with the document
        for world, repl in ((1, -1), (3, -1), (3, 0)):
            n = c if repl == 0 else c * world
            (b,), final, inbox = _parse_sync(_run(check_exe, _sync(
                40000, world, world - 1, ms, repl, [("equal", 8, 8 + n)])))
            assert (b["owner"], b["lo"], b["c"], b["rslot"], b["nruns"]) == (-1, 8, c, c, 0)
            assert _cut(c, b["slice"], b["nslice"]) == want, (c, ms, b)
            assert final[0] == (len(want), -1) and set(final[1:]) == {(0, -1)}
            assert inbox == c * world * (2 if repl == 0 else 1)
    for runs, ms, want, first in RUN_SETS:
        assert owner_slices(runs, ms) == (want, first)
        # out of order and non-adjacent in the plan buffer, state offsets shuffled
        los = [20000 - 6000 * i for i in range(len(runs))] if len(runs) < 8 else \
            [8 * i for i in range(8)]
        soffs = [5200 * ((i * 5 + 2) % len(runs)) for i in range(len(runs))]
        spec = ("owner", [(lo, lo + n) for lo, n in zip(los, runs)], soffs, 1)
        (b,), final, inbox = _parse_sync(_run(check_exe, _sync(30000, 2, 0, ms, -1, [spec])))
        per = b["slice"]
        got = sum((_cut(n, per, (n + per - 1) // per) for n in runs), [])
        assert got == want and b["nslice"] == len(want) == first[-1]
        assert [r[5] for r in b["runs"]] + [b["end"]] == first
        voff = [sum(runs[:i]) for i in range(len(runs))]
        assert b["runs"] == [(lo, n, so, vo, per, f)
                             for lo, n, so, vo, f in zip(los, runs, soffs, voff, first)]
        assert (b["owner"], b["lo"], b["c"], b["rslot"]) == (1, los[0], sum(runs), 0)
        assert final[0] == (len(want), 1) and inbox == 2 * sum(runs)
    for sizes, ms, want in SHARD_SETS:
        assert [len(async_slices(n, ms)) for n in sizes] == want
        los = [sum(sizes[:i]) + 8 for i in range(len(sizes))]
        rows = _run(check_exe, _async(20480, 1, 0, ms, [(lo, lo + n) for lo, n in zip(los, sizes)],
                                      [0] * len(sizes)))
        assert [r[0] for r in rows] == ["shard"] * len(sizes) + ["inbox"]
        for i, r in enumerate(rows[:-1]):
            lo, n, host, slice_, nslice, slice0, inbox_off = map(int, r[1:])
            assert (lo, n, host) == (los[i], sizes[i], 0)
            assert _cut(n, slice_, nslice) == async_slices(n, ms)
            assert slice0 == sum(want[:i]) and inbox_off == sum(sizes[:i])
        assert int(rows[-1][1]) == sum(sizes)


def test_slice_rule_sweep(check_exe):
    cells = [(n, per_wg, ms) for per_wg in (1024, 2048) for ms in (1, 2, 128, 512)
             for n in range(4, 8197, 4)]
    rows = _run(check_exe, "".join("geo %d %d %d 1\n" % c for c in cells))
    assert len(rows) == len(cells)
    for (n, per_wg, ms), r in zip(cells, rows):
        twin = equal_slices(n, ms) if per_wg == 1024 else async_slices(n, ms)
        assert _cut(n, int(r[1]), int(r[2])) == twin, (n, per_wg, ms, r)
    # the owner form: the slice count raised to the run count
    rows = _run(check_exe, "geo 5040 1024 1 2\ngeo 32 1024 128 8\n")
    assert rows == [["geo", "2520", "2"], ["geo", "4", "8"]]


def test_mixed_plan_inbox_offsets(check_exe):
    world, ms = 3, 128
    owner_runs, soffs = [(12000, 13028), (40, 44), (9000, 11052)], [2056, 0, 4]
    buckets = [("owner", owner_runs, soffs, 2), ("equal", 1000, 1000 + 3 * 1028),
               ("owner", [(16000, 16400)], [0], 0), ("equal", 5000, 8076)]
    twin = [("owner", owner_runs, soffs, 2), ("equal", 1000, 1000 + 3 * 1028, 0),
            ("owner", [(16000, 16400)], [0], 0), ("equal", 5000, 8076, 0)]
    sizes = [3084 * world, 1028 * world, 400 * world, 3076 * world * 2]  # replicated: 2 parities
    for rank in range(world):
        got, final, inbox = _parse_sync(_run(check_exe, _sync(20480, world, rank, ms, 3, buckets)))
        assert [b["inbox_off"] for b in got] == [sum(sizes[:i]) for i in range(4)]
        assert inbox == sum(sizes)
        assert [f[1] for f in final[:5]] == [2, -1, 0, -1, -1]
        assert [f[0] for f in final[:4]] == [b["nslice"] for b in got]
        # the spans this rank updates, as the GPU tests' twin lists them
        for b, tw, repl in zip(got, twin, (False, False, False, True)):
            mine = bucket_regions(tw, world, repl)[rank]
            if tw[0] == "owner":
                spans = [(lo, n, so) for lo, n, so, _, _, _ in b["runs"]] if rank == tw[3] else []
            elif repl:
                spans = [(b["lo"], b["c"], 0)]
            else:
                spans = [(b["lo"] + rank * b["c"], b["c"], 0)]
            assert spans == mine
    # an async plan over three hosts: every host's inbox in PS order, whichever rank computes it
    sizes, hosts = [4, 2052, 4100, 2044], [0, 2, 2, 1]
    ranges = [(8, 12), (12, 2064), (4000, 8100), (9000, 11044)]
    for rank in range(3):
        rows = _run(check_exe, _async(20480, 3, rank, 512, ranges, hosts))
        assert [int(r[7]) for r in rows[:-1]] == [0, 0, 2052 * 3, 0]
        assert [int(r[6]) for r in rows[:-1]] == [0, 1, 3, 6]
        assert int(rows[-1][1]) == 3 * sum(n for n, h in zip(sizes, hosts) if h == rank)


def test_refusals(check_exe):
    eq = [("equal", 0, 4096)]
    own = lambda runs, soffs=None, owner=0: [("owner", runs, soffs or [0] * len(runs), owner)]
    big = 1 << 40
    sync = [
        (_sync(4096, 0, 0, 8, -1, eq), "xgmi: world out of range"),
        (_sync(4096, 17, 0, 8, -1, eq), "xgmi: world out of range"),
        (_sync(4096, 2, 2, 8, -1, eq), "xgmi: rank out of range"),
        (_sync(4096, 2, 0, 8, -1, []), "xgmi: 1..32 buckets"),
        (_sync(4096, 1, 0, 8, -1, [("equal", 0, 4)] * 33), "xgmi: 1..32 buckets"),
        (_sync(4096, 2, 0, 0, -1, eq), "xgmi: max_slices out of range"),
        (_sync(4096, 2, 0, 513, -1, eq), "xgmi: max_slices out of range"),
        (_sync(4096, 2, 0, 8, 1, eq), "xgmi: replicated bucket"),
        (_sync(4096, 2, 0, 8, -1, own([(0, 8)], owner=2)), "xgmi: bucket owner out of range"),
        (_sync(4096, 2, 0, 8, 0, own([(0, 8)])), "xgmi: an owner bucket cannot be replicated"),
        (_sync(4096, 2, 0, 8, -1, own([(4 * i, 4 * i + 4) for i in range(9)])),
         "xgmi: owner bucket needs 1..8 runs with state offsets"),
        (_sync(4096, 2, 0, 8, -1, own([(0, 4100)])),
         "xgmi: owner-bucket run out of range or not 16-B shaped"),
        (_sync(4096, 2, 0, 8, -1, own([(2, 10)])),
         "xgmi: owner-bucket run out of range or not 16-B shaped"),
        (_sync(4096, 2, 0, 8, -1, own([(0, 8)], [2])),
         "xgmi: owner-bucket run out of range or not 16-B shaped"),
        (_sync(big, 2, 0, 512, -1,
               own([(70000 * i, 70000 * i + 65536 + (4 if i % 2 else -4)) for i in range(8)])),
         "xgmi: owner bucket has too many slices"),
        (_sync(big, 2, 0, 8, -1, own([(0, 1 << 28)])), "xgmi: bucket too large"),
        ("sync 4096 2 0 8 -1 1\n-1 2 0 8 8 16\n", "xgmi: equal-chunk bucket needs one range"),
        (_sync(4096, 2, 0, 8, -1, [("equal", 0, 4104)]), "xgmi: bucket out of range"),
        (_sync(4096, 2, 0, 8, -1, [("equal", 8, 8)]), "xgmi: bucket out of range"),
        (_sync(4096, 3, 0, 8, -1, [("equal", 0, 16)]),
         "xgmi: bucket not divisible by 4W (replicated: by 4)"),
        (_sync(4096, 3, 0, 8, 0, [("equal", 0, 18)]),
         "xgmi: bucket not divisible by 4W (replicated: by 4)"),
        (_sync(big, 2, 0, 8, -1, [("equal", 0, 1 << 29)]), "xgmi: bucket too large"),
        (_sync(big, 2, 0, 8, 0, [("equal", 0, 1 << 27)]), "xgmi: bucket too large"),
    ]
    one = [(0, 4096)]
    asyn = [
        (_async(4096, 0, 0, 8, one, [0]), "async xgmi: world"),
        (_async(4096, 2, -1, 8, one, [0]), "async xgmi: rank"),
        (_async(4096, 2, 0, 8, [], []), "async xgmi: 1..64 PS, one host each"),
        (_async(4096, 2, 0, 8, [(4 * i, 4 * i + 4) for i in range(65)], [0] * 65),
         "async xgmi: 1..64 PS, one host each"),
        (_async(4096, 2, 0, 8, one, [0, 1]), "async xgmi: 1..64 PS, one host each"),
        (_async(4096, 2, 0, 0, one, [0]), "async xgmi: max_slices"),
        (_async(4096, 2, 0, 513, one, [0]), "async xgmi: max_slices"),
        (_async(4096, 2, 0, 8, [(0, 4100)], [0]),
         "async xgmi: PS range must be a 4-aligned slice of the buffer"),
        (_async(4096, 2, 0, 8, [(2, 6)], [0]),
         "async xgmi: PS range must be a 4-aligned slice of the buffer"),
        (_async(4096, 2, 0, 8, [(8, 8)], [0]),
         "async xgmi: PS range must be a 4-aligned slice of the buffer"),
        (_async(4096, 2, 0, 8, one, [2]), "async xgmi: PS host"),
        (_async(big, 2, 0, 8, [(0, 1 << 28)], [0]), "async xgmi: shard too large"),
    ]
    cases = sync + asyn
    rows = _run(check_exe, "".join(text for text, _ in cases))
    assert [" ".join(r) for r in rows] == ["refused " + msg for _, msg in cases]
    # the same shapes just inside the bounds are planned
    ok = _run(check_exe, _sync(4096, 16, 15, 512, 0, [("equal", 0, 4096)] * 32) +
              _sync(big, 2, 0, 8, -1, [("equal", 0, (1 << 29) - 8)]) +
              _sync(big, 2, 0, 512, -1, own([(70000 * i, 70000 * i + 65536) for i in range(8)])) +
              _async(4096, 16, 15, 512, [(4 * i, 4 * i + 4) for i in range(64)], [15] * 64))
    assert not [r for r in ok if r[0] == "refused"]
    assert [r for r in ok if r[0] == "inbox"][-1] == ["inbox", str(64 * 4 * 16)]
