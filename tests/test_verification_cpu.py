"""Identity verification without a GPU: the float64 oracle against outputs recorded from the reference's own functions (pyeer's
get_eer_stats, the two split_gen_imp samplers), the package's pair lists against the same recordings, grouping, and every refusal."""
import json
import os
import re

import numpy as np
import pytest

import verification_oracle as O
from faceposegenerator_amd import _lib
from faceposegenerator_amd import verification as V

HERE = os.path.dirname(os.path.abspath(__file__))
PYEER = json.load(open(os.path.join(HERE, "golden", "verification_pyeer.json")))
PAIRS = np.load(os.path.join(HERE, "golden", "verification_pairs.npz"))
EXACT = ("eer", "eer_low", "eer_high", "eer_th", "fmr0", "fmr1000", "fmr100", "fmr20", "fmr10", "fnmr0", "fnmr100", "fnmr1000", "fmr0_th",
         "fmr1000_th", "fmr100_th", "fmr20_th", "fmr10_th", "fnmr0_th", "j_index", "j_index_th", "mccoef_th")


def test_golden_covers_the_cases():
    assert sorted(PYEER) == sorted(O.SCORE_CASES)
    assert PYEER["all_equal"]["eer"] == 1.0 and PYEER["no_crossing"]["eer"] == 1.0 and PYEER["perfect"]["eer"] == 0.0
    assert PYEER["inverted"]["eer"] > 0.9 and (PYEER["single"]["ng"], PYEER["single"]["ni"]) == (1, 1)


@pytest.mark.parametrize("case", O.SCORE_CASES)
def test_oracle_matches_recorded_pyeer(case):
    g, i = O.score_case(case)
    want, got = PYEER[case], O.stats(g, i)
    assert (len(g), len(i), got["_"]["n_thresholds"]) == (want["ng"], want["ni"], want["n_thresholds"])
    for key in EXACT:
        assert got[key] == want[key], (key, got[key], want[key])
    assert abs(got["auc"] - want["auc"]) <= 1e-12
    assert got["mccoef"] == pytest.approx(want["mccoef"], rel=0, abs=1e-15)
    for key in ("gmean", "gstd", "imean", "istd"):
        assert got[key] == want[key], key
    if np.isfinite(want["decidability"]):
        assert got["decidability"] == want["decidability"]


@pytest.mark.parametrize("case", O.SCORE_CASES)
def test_mcc_fixture_has_a_clear_maximum(case):
    assert O.stats(*O.score_case(case))["_"]["mcc_gap"] > 1e-9


def test_host_statistics_from_kernel_outputs_match_the_oracle():
    """stats_from_roc is the host half of eer_stats: fed the oracle's own points, it reproduces every scalar."""
    for case in O.SCORE_CASES:
        g, i = O.score_case(case)
        want = O.stats(g, i)
        aux = want["_"]
        names = _lib.IDB_VERIF_POINTS
        points = np.array([aux["points"].get(n, (np.nan, -1, -1))[0] for n in names])
        ints = np.array([v for n in names for v in aux["points"].get(n, (np.nan, -1, -1))[1:]] + [aux["n_thresholds"], aux["n_le0"], aux["auc2"]],
                        dtype=np.int64)
        moments = np.array([want["gmean"], want["gstd"], want["imean"], want["istd"]])
        got = V.stats_from_roc(points, ints, moments, len(g), len(i))
        for key, val in got.items():
            assert val == want[key] or (np.isnan(val) and np.isnan(want[key])), (case, key, val, want[key])
        assert set(got) == set(want) - {"_"}


def test_pairs_among_synth_match_the_reference():
    got = V.pairs_among_synth(PAIRS["counts_synth"])
    for arr, name in zip(got, ("among_gen_a", "among_gen_b", "among_imp_a", "among_imp_b")):
        assert arr.dtype == np.int32 and np.array_equal(arr, PAIRS[name]), name
    for arr, ref in zip(O.pairs(list(PAIRS["counts_synth"]), None, 0, 8, 18), got):
        assert np.array_equal(arr, ref)


def test_pairs_synth_vs_real_match_the_reference():
    got = V.pairs_synth_vs_real(PAIRS["counts_synth"], PAIRS["counts_real"])
    for arr, name in zip(got, ("real_gen_a", "real_gen_b", "real_imp_a", "real_imp_b")):
        assert arr.dtype == np.int32 and np.array_equal(arr, PAIRS[name]), name
    for arr, ref in zip(O.pairs(list(PAIRS["counts_synth"]), list(PAIRS["counts_real"]), 0, 8, 17), got):
        assert np.array_equal(arr, ref)


def test_pair_fixture_covers_the_sizes():
    cs, cr = PAIRS["counts_synth"], PAIRS["counts_real"]
    assert len(cs) == len(cr) and len(cs) % 18 and len(cs) % 17 and (cs != cr).any()
    for c in (cs, cr):
        assert (c == 1).any() and ((c > 1) & (c < 8)).any() and (c == 8).any() and (c > 8).any()


def test_pairs_do_not_touch_global_random_state():
    import random
    random.seed(5)
    np.random.seed(5)
    want = (random.random(), np.random.rand())
    random.seed(5)
    np.random.seed(5)
    V.pairs_among_synth([3, 9, 2, 8])
    assert (random.random(), np.random.rand()) == want


def test_grouping_order_and_valid():
    names = ["d/10_0.png", "d/2_0.png", "1_0.png", "d/10_1.png", "1-2_0.png", "d/1_1.png", "d/2_1.png"]
    embs = np.arange(len(names), dtype=np.float32).reshape(-1, 1) * np.ones((1, 4), dtype=np.float32)
    out, counts, ids = V.group_by_identity(embs, names)
    assert ids == ["1-2", "1", "10", "2"]                    # sorted("<id>.npy"): '-' < '.' < '0'
    assert counts.tolist() == [1, 2, 2, 2] and out[:, 0].tolist() == [4, 2, 5, 0, 3, 1, 6]
    order, ocounts, oids = O.group_by_identity(names)
    assert (order, ocounts, oids) == ([4, 2, 5, 0, 3, 1, 6], [1, 2, 2, 2], ids)
    valid = [True, False, True, True, False, True, False]
    out, counts, ids = V.group_by_identity(embs, names, valid)
    assert ids == ["1", "10"] and counts.tolist() == [2, 2] and out[:, 0].tolist() == [2, 5, 0, 3]


def test_refusals():
    e = np.ones((4, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        V.group_by_identity(e, ["a_0", "a_1"])
    with pytest.raises(ValueError):
        V.group_by_identity(np.ones(4), ["a_0"] * 4)
    with pytest.raises(ValueError):
        V.group_by_identity(e, ["a_0"] * 4, valid=[True])
    with pytest.raises(ValueError):
        V.group_by_identity(e, ["a_0"] * 4, valid=[False] * 4)
    with pytest.raises(ValueError):
        V.pairs_among_synth([])
    with pytest.raises(ValueError):
        V.pairs_among_synth([3, 0])
    with pytest.raises(ValueError):
        V.pairs_among_synth([3.0, 2.0])
    with pytest.raises(ValueError):
        V.pairs_among_synth([3, 2], samples_skip=0)
    with pytest.raises(ValueError):
        V.pairs_synth_vs_real([3, 2], [3, 2, 4])
    with pytest.raises(ValueError):
        V.cos_scores(e, np.ones((4, 7), dtype=np.float32), [0], [0])
    with pytest.raises(ValueError):
        V.cos_scores(e.astype(np.int32), e, [0], [0])
    with pytest.raises(ValueError):
        V.cos_scores(e, e, [0, 4], [0, 1])
    with pytest.raises(ValueError):
        V.cos_scores(e, e, [0, 1], [0])
    with pytest.raises(ValueError):
        V.cos_scores(e, e, [], [])
    with pytest.raises(ValueError):
        V.cos_scores(e, e, [0.5], [0.5])
    with pytest.raises(ValueError):
        V.eer_stats(np.zeros(0), np.ones(3))
    with pytest.raises(ValueError):
        V.eer_stats(np.array([0.1, np.nan]), np.ones(3))
    with pytest.raises(ValueError):
        V.eer_stats(np.ones((2, 2)), np.ones(3))
    with pytest.raises(ValueError):
        V.verification_report(e, ["a_0"] * 4, real_embs=e)
    with pytest.raises(ValueError):
        V.verification_report(e, ["a_0", "a_1", "a_2", "a_3"])           # one identity: no impostor pair


def test_library_refuses_bad_arguments_before_any_hip_call(lib):
    assert lib.idb_verif_workspace_bytes(0, 5) == 0 and lib.idb_verif_workspace_bytes(5, (1 << 30) + 1) == 0
    assert lib.idb_verif_workspace_bytes(1, 1) > 0
    assert lib.idb_verif_cos_scores(0x1000, 4, 0x1000, 4, 0, 0x1000, 0x1000, 1, 0x1000, None) == -1
    assert lib.idb_verif_cos_scores(0x1000, 4, 0x1000, 4, 8, 0x1000, 0x1000, 0, 0x1000, None) == -1
    assert lib.idb_verif_cos_scores(0x1000, 4, None, 4, 8, 0x1000, 0x1000, 1, 0x1000, None) == -1
    assert b"null" in lib.idb_last_error()
    assert lib.idb_verif_roc(0x1000, 0, 0x1000, 4, 0x1000, 0x1000, 0x1000, 0x1000, 1 << 20, None) == -1
    assert lib.idb_verif_roc(0x1000, 4, 0x1000, 4, 0x1000, 0x1000, 0x1000, 0x1000, 8, None) == -1
    assert b"workspace" in lib.idb_last_error()
    assert lib.idb_verif_roc(0x1000, 4, 0x1000, 4, 0x1000, 0x1000, 0x1000, 0x1008, 1 << 20, None) == -1


def test_symbols_in_header_and_binding():
    txt = open(os.path.join(os.path.dirname(HERE), "include", "idb_kernels.h")).read()
    for name in ("idb_verif_cos_scores", "idb_verif_workspace_bytes", "idb_verif_roc"):
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS
    assert len(_lib.IDB_VERIF_POINTS) == int(re.search(r"#define IDB_VERIF_POINTS (\d+)", txt).group(1))
    for k, name in enumerate(_lib.IDB_VERIF_POINTS):
        macro = {"youden": "YOUDEN", "mcc": "MCC", "first": "FIRST"}.get(name, name.upper())
        assert int(re.search(r"#define IDB_VERIF_%s (\d+)" % macro, txt).group(1)) == k
