"""The general (non-layout) two-graph window pass -- the build every table outside the layout-order
limits takes -- pinned on its own: MR_NO_LO_WIN=1 throughout, so win_chunk_build_async goes to
mr_ix_launch2_batch (and, under MR_NO_IX2, to a build per mask) on tables small enough to test
every chunk shape and both detector placements in well under a second."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("MR_WIN_CHUNK", "MR_WIN_GROUP", "MR_NO_DET_FUSE", "MR_DET_FUSE_MAX", "MR_NO_IX2", "MR_IX_EPT", "MR_EDGE_HASH",
         "MR_NO_INDEX")
# (seed, traces): 40 ops each.  300 traces: one 2048-trace selection tile, two 256-trace detector
# tiles, a multiple of neither; 2500: two selection tiles unfused, ten fused (the look-back chains
# cross tiles); 700: between them, and with 300 below MR_DET_FUSE_MAX=1000 while 2500 is above.
TABLES = ((501, 300), (502, 2500), (503, 700))
VARIANTS = {
    "default": {},   # (five windows: chunks of 4 and 1)
    "chunk1": {"MR_WIN_CHUNK": "1"},
    "chunk2": {"MR_WIN_CHUNK": "2"},
    "chunk8": {"MR_WIN_CHUNK": "8"},   # one batch of all five: the empty window inside a multi-window batch
    "nofuse": {"MR_NO_DET_FUSE": "1"},
    "nofuse_chunk1": {"MR_NO_DET_FUSE": "1", "MR_WIN_CHUNK": "1"},
    "fuse_split": {"MR_DET_FUSE_MAX": "1000"},   # a chunk whose windows disagree on fusion
    "fuse_split_chunk2": {"MR_DET_FUSE_MAX": "1000", "MR_WIN_CHUNK": "2"},
    "per_mask": {"MR_NO_IX2": "1"},
}
MIN5 = 5 * 60 * 10**9


@pytest.fixture(scope="module")
def general_pass_runs():
    """Five windows (one per table over its 5-minute span, the 2500-trace table again a minute
    later, an empty window) ranked once per variant; the C oracle's window for each non-empty one."""
    import bench
    import c_oracle
    from microrank_amd import _lib
    from microrank_amd.online_rca import rank_windows
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    tabs, wins, devs = [], [], []
    for seed, n_traces in TABLES:
        _, normal, ab = bench.make_window(seed, 40, n_traces)
        a3, ok = bench.slo_from_gpu(ctx, normal)
        d = DeviceSpans(ctx, ab)
        devs.append(d)
        t0 = int(ab.tstart.min())
        tabs.append(ab)
        wins.append((d, t0, t0 + MIN5, a3, ok))
    tabs.append(tabs[1])
    wins.append((wins[1][0], wins[1][1] + 60 * 10**9, wins[1][2] + 60 * 10**9, wins[1][3], wins[1][4]))
    wins.append((wins[0][0], 0, 1, wins[0][3], wins[0][4]))   # no trace in [0, 1] ns: empty window
    mp = pytest.MonkeyPatch()
    runs = {}
    try:
        for name, env in VARIANTS.items():
            for k in KNOBS:
                mp.delenv(k, raising=False)
            mp.setenv("MR_NO_LO_WIN", "1")
            for k, v in env.items():
                mp.setenv(k, v)
            runs[name] = rank_windows(ctx, wins)
    finally:
        mp.undo()
    refs = [c_oracle.rca_window(st, w[1], w[2], w[3], w[4], nthreads=0) for st, w in zip(tabs, wins[:4])]
    yield runs, refs
    for d in devs:
        d.close()


def test_tables_span_the_tile_sizes():
    """The shapes the cases are chosen for (SEL_TILE = 2048 traces, the detector's 256)."""
    n = [t for _, t in TABLES]
    assert n[0] < 2048 and 256 < n[0] < 512 and n[0] % 256
    assert n[1] > 2048 and n[1] % 2048 and n[1] % 256
    assert n[0] < 1000 and n[2] < 1000 < n[1]


def test_windows_are_ranked_and_empty_window_is_flagged(general_pass_runs):
    from microrank_amd import _lib

    runs, _ = general_pass_runs
    for name, got in runs.items():
        assert len(got) == 5
        for i, (codes, scores, na, nn, edges, status) in enumerate(got[:4]):
            assert status == 0, (name, i)
            assert na > 0 and nn > 0, (name, i)
            assert len(codes) == len(scores) > 0 and edges > 0, (name, i)
        assert got[4][5] == _lib.MR_ERR_VALUE, name


@pytest.mark.parametrize("name", [v for v in VARIANTS if v not in ("default", "per_mask")])
def test_build_side_choices_rank_bitwise(general_pass_runs, name):
    """Chunk sizes, the detector's placement (fused, its own launch, mixed within a chunk): status,
    (na, nn, edges), top list and score bytes equal the default's."""
    runs, _ = general_pass_runs
    for i, (a, b) in enumerate(zip(runs["default"], runs[name])):
        assert a[5] == b[5], i
        assert a[2:] == b[2:] and list(a[0]) == list(b[0]), i
        assert a[1].tobytes() == b[1].tobytes(), i


def test_build_per_mask_agrees(general_pass_runs):
    """MR_NO_IX2 (detector, masks, one indexed build per graph): counts, edges and lists equal,
    scores within 1e-12."""
    runs, _ = general_pass_runs
    for i, (a, b) in enumerate(zip(runs["default"], runs["per_mask"])):
        assert a[5] == b[5], i
        assert (a[2], a[3], a[4]) == (b[2], b[3], b[4]), i
        assert list(a[0]) == list(b[0]), i
        np.testing.assert_allclose(a[1], b[1], rtol=1e-12, atol=0, err_msg=f"window {i}")


def test_default_matches_c_oracle(general_pass_runs):
    """Every non-empty window against the C restatement of the driver's window: counts, edges and
    the 11 codes equal, DStar2 scores within 1e-10."""
    runs, refs = general_pass_runs
    for i, ref in enumerate(refs):
        codes, scores, na, nn, edges, status = runs["default"][i]
        rc, rs, rna, rnn, redges = ref
        assert status == 0, i
        assert (na, nn) == (rna, rnn), i
        assert na > 0 and nn > 0 and len(rc) == 11
        assert edges == redges, i
        assert list(codes) == list(rc), i
        np.testing.assert_allclose(scores, rs, rtol=1e-10, atol=0, err_msg=f"window {i}")
