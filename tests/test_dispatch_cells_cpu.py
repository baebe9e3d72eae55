"""The cell table of tests/test_dispatch_oracle_gpu.py (tests/dispatch_cells.py), without a GPU:
every cell names at least one branch and only known ones, and every branch name is expected by
some cell (the GPU test holds BRANCHES against the engine's own dispatch_hits().keys())."""
import dispatch_cells as D


def test_every_cell_names_its_branches():
    cells = D.all_expectations()
    assert len({name for name, _ in cells}) == len(cells)   # cell names are unique
    for name, want in cells:
        assert want, name
        assert set(want) <= set(D.BRANCHES), name
        assert all(v >= 1 for v in want.values()), name
        # one launch choice per pair and segment, and a tail leaves exactly once per segment
        tails = want.get("tail_standalone", 0) + want.get("tail_consumed", 0)
        assert tails == (name.startswith("tail: ") + 2 * name.startswith("chain + tails: ")), name


def test_every_branch_is_expected_by_some_cell():
    assert len(set(D.BRANCHES)) == len(D.BRANCHES)
    seen = set()
    for _, want in D.all_expectations():
        seen |= set(want)
    assert [b for b in D.BRANCHES if b not in seen] == []


def test_each_tail_cell_reaches_the_branch_it_names():
    """TAIL_CELLS has one schedule per launch choice of segments 1-3 and the two-stream mode."""
    firsts = [next(iter(D.expected_hits(s, sched, 6272, tail=True)[0])) for s, _, sched in D.TAIL_CELLS]
    assert firsts == ["conv4_dual_tail", "conv4_back_to_back", "conv3_dual", "conv3_back_to_back",
                      "tail_consumed", "tail_consumed", "tail_consumed", "tail_consumed",
                      "seg3_unfused", "seg3_unfused", "concurrent"]
    exits = [set(D.expected_hits(3, sched, 6272)[0]) for s, _, sched in D.TAIL_CELLS if s == 3]
    assert exits == [{"seg3_direct_reduce"}, {"seg3_direct"}, {"seg3_reduce_gemm"},
                     {"seg3_reduce_refused"}, {"seg3_unfused", "conv2_dual"},
                     {"seg3_unfused", "conv2_back_to_back"}]


def test_split_counts_follow_gemm_h():
    """splitk_z: K over the chunk rounded up to whole K tiles."""
    assert D.splitk_z(512, 3, 32) == 3 and D.splitk_z(512, 1, 32) == 1
    assert D.splitk_z(6400, 3, 32) == 3 and D.splitk_z(1600, 3, 16) == 3
    assert D.splitk_z(6272, 48, 32) == 40 and D.splitk_z(6272, 12, 16) == 12
    assert D.mode_of(6272, 48, 1, 32) == 2 and D.mode_of(6272, 48, 1 << 20, 32) == 1
    assert D.mode_of(6272, 1, 1, 32) == 0
