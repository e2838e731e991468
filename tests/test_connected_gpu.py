"""GPU: connected-word recognition (csrc/connected.hip) through the C ABI and the Python layer against the CPU
restatement tests/_connected_ref.py.

Measured on an MI355X (the figures DESIGN.md section 5 records): recursion — every output equal to the reference on
all 42 (shape, topology, exit set) cases; emission — largest relative difference from numpy 9.0e-16 (bound 1e-13);
end to end — every path and entry flag equal, largest relative score difference 2.1e-16 (bound 1e-12)."""
import pickle

import numpy as np
import pytest

from tests import _connected_ref as ref

pytestmark = pytest.mark.gpu

NEG = -np.inf
SHAPES = [(3, 4), (11, 10), (11, 18), (14, 18), (64, 4), (5, 7), (2, 1),
          (3, 12), (17, 3), (4, 11),   # RL = 1, 2, 2 at SP = 18, 4, 18: shapes the lists of the sibling decoders share
          (25, 10)]                    # ... and (RL, SP) = (4, 10)
LENGTHS = [3, 64, 1, 300, 0, 65, 2, 63]   # mixed within one batch, an empty utterance in the middle


def _network(rng, W, S, topology, exits, integer):
    """(log_start, log_trans, log_exit): bidiagonal, with an i -> i + 2 skip, or dense; integer-valued tables
    (log_trans in {0, -1, -inf}) are full of ties."""
    width = {"bidiag": 1, "skip": 2, "dense": S}[topology]
    lt = np.full((W, S, S), NEG)
    ls = np.full((W, S), NEG)
    for i in range(S):
        lo = 0 if topology == "dense" else i
        for j in range(lo, min(S, i + width + 1)):
            lt[:, i, j] = -rng.integers(0, 2, W) if integer else np.log(rng.uniform(0.05, 1.0, W))
            if integer and j != i:   # -inf inside the band too (the self-loop stays: every word can go on)
                lt[rng.random(W) < 0.2, i, j] = NEG
    n_start = S if topology == "dense" else min(S, 2)
    ls[:, :n_start] = -rng.integers(0, 2, (W, n_start)) if integer else np.log(rng.uniform(0.05, 1.0, (W, n_start)))
    lx = np.full((W, S), NEG)
    if exits == "last":
        lx[:, S - 1] = 0.0
    else:
        lx[:] = 0.0
    return ls, lt, lx


def _assert_equal(res, want, what):
    score, n_words, pw, ps, pe = want
    assert np.array_equal(res.score, score), what               # (bit-equal: -inf == -inf, no NaN in these cases)
    assert np.array_equal(res.n_words, n_words), what
    assert np.array_equal(res.path_word, pw), what
    assert np.array_equal(res.path_state, ps), what
    assert np.array_equal(res.path_entry, pe), what


@pytest.mark.parametrize("exits", ["last", "any"])
@pytest.mark.parametrize("topology", ["bidiag", "dense", "skip"])
@pytest.mark.parametrize("W,S", SHAPES)
def test_recursion_equals_reference(W, S, topology, exits):
    from sapr_amd.connected import ConnectedNetwork, connected_viterbi
    rng = np.random.default_rng(7 * W + S)
    total = sum(LENGTHS)
    for integer in (False, True):
        ls, lt, lx = _network(rng, W, S, topology, exits, integer)
        logb = (-rng.integers(0, 4, (total, W, S)).astype(np.float64) if integer
                else rng.normal(-40.0, 15.0, (total, W, S)))
        for pen in (0.0, -20.0, 3.0):
            net = ConnectedNetwork(ls, lt, lx, word_penalty=pen)
            res = connected_viterbi(logb, LENGTHS, net)
            want = ref.viterbi_batch(logb, LENGTHS, ls, lt, lx, pen)
            _assert_equal(res, want, (integer, pen))
            assert res.score[LENGTHS.index(0)] == NEG and res.n_words[LENGTHS.index(0)] == 0
            if exits == "any":
                assert np.isfinite(res.score[np.asarray(LENGTHS) > 0]).all()


def test_recursion_ignores_the_padded_columns_of_logb():
    """(5, 7) runs in SP = 10: whatever finite value the caller leaves in the three padded columns changes nothing."""
    from sapr_amd.connected import ConnectedNetwork, connected_viterbi
    rng = np.random.default_rng(3)
    W, S, SP = 5, 7, 10
    ls, lt, lx = _network(rng, W, S, "skip", "last", False)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    wide = rng.normal(50.0, 5.0, (sum(LENGTHS), W, SP))
    wide[:, :, :S] = logb
    net = ConnectedNetwork(ls, lt, lx, word_penalty=-1.5)
    want = ref.viterbi_batch(logb, LENGTHS, ls, lt, lx, -1.5)
    _assert_equal(connected_viterbi(wide, LENGTHS, net), want, "wide")
    _assert_equal(connected_viterbi(wide.reshape(-1, W * SP), LENGTHS, net), want, "flat")


def test_no_reachable_exit_scores_minus_infinity():
    """Bidiagonal words that start in state 0 and may end in their last state only: T < S frames reach no exit."""
    from sapr_amd.connected import ConnectedNetwork, connected_viterbi
    rng = np.random.default_rng(5)
    W, S = 11, 10
    ls, lt, lx = _network(rng, W, S, "bidiag", "last", False)
    ls[:, 1:] = NEG
    lengths = [1, 9, 10, 3, 25]
    logb = rng.normal(-40.0, 15.0, (sum(lengths), W, S))
    res = connected_viterbi(logb, lengths, ConnectedNetwork(ls, lt, lx))
    _assert_equal(res, ref.viterbi_batch(logb, lengths, ls, lt, lx, 0.0), "unreachable")
    for u in (0, 1, 3):
        lo, hi = res.offsets[u], res.offsets[u + 1]
        assert res.score[u] == NEG and res.n_words[u] == 0 and res.segments(u) == []
        assert (res.path_word[lo:hi] == -1).all() and (res.path_state[lo:hi] == -1).all()
        assert not res.path_entry[lo:hi].any()
    assert np.isfinite(res.score[[2, 4]]).all() and res.n_words[2] == 1


def test_single_state_words_stay_on_exact_ties():
    """(2, 1) with penalty 0 and equal scores: "stay" and "re-enter" tie exactly; stay wins, and word 0 wins E."""
    from sapr_amd.connected import ConnectedNetwork, connected_viterbi
    z = np.zeros((2, 1))
    net = ConnectedNetwork(z, np.zeros((2, 1, 1)), z, word_penalty=0.0)
    res = connected_viterbi(np.zeros((12, 2, 1)), [5, 7], net)
    assert res.score.tolist() == [0.0, 0.0] and res.n_words.tolist() == [1, 1]
    assert (res.path_word == 0).all() and (res.path_state == 0).all()
    assert res.path_entry.tolist() == [1, 0, 0, 0, 0] + [1, 0, 0, 0, 0, 0, 0]
    assert res.segments(1) == [(0, 0, 7)]
    # a positive penalty makes re-entering strictly better at every frame
    res = connected_viterbi(np.zeros((12, 2, 1)), [5, 7], ConnectedNetwork(z, np.zeros((2, 1, 1)), z, 3.0))
    assert res.score.tolist() == [12.0, 18.0] and res.n_words.tolist() == [5, 7] and res.path_entry.all()


def _gauss_network(rng, W, S, D):
    from sapr_amd.connected import ConnectedNetwork
    means = rng.normal(0.0, 20.0, (W, S, D))
    vars_ = rng.uniform(1.0, 36.0, (W, S, D))
    gconst = D * np.log(2 * np.pi) + np.log(vars_).sum(axis=-1)
    z = np.zeros((W, S))
    return ConnectedNetwork(z, np.zeros((W, S, S)), z, 0.0, None, means, vars_, gconst)


@pytest.mark.parametrize("W,S,D", [(3, 4, 5), (11, 10, 13), (5, 7, 26), (11, 18, 39), (2, 1, 1)])
def test_emission_matches_numpy(W, S, D):
    """rtol 1e-13: every term of the sum is non-negative and gconst > 0 for variances >= 1, so nothing cancels; each
    term is off by a few ulp (the reciprocal form adds one rounding) and the sum by D more: below 1e-14."""
    import torch
    from sapr_amd.connected import emit_diag
    rng = np.random.default_rng(11 * W + D)
    net = _gauss_network(rng, W, S, D)
    worst = 0.0
    for total in (1, 255, 257, 1000):
        x = rng.normal(0.0, 20.0, (total, D)).astype(np.float32)
        got = emit_diag(torch.from_numpy(x).cuda(), net).cpu().numpy().reshape(total, W, net.SP)
        want = ref.emit_diag(x, net.means, net.vars, net.gconst)
        assert np.all(got[:, :, S:] == NEG)                      # padded columns
        rel = np.abs(got[:, :, :S] - want) / np.abs(want)
        worst = max(worst, float(rel.max()))
        print(f"emission ({W}, {S}, {D}) x {total} frames: max relative difference {rel.max():.3g}")
        assert rel.max() <= 1e-13
    assert worst <= 1e-13


def _reference_decode(model, utts, pen=0.0):
    logb = np.concatenate([ref.emit_diag(x, model["means"], model["vars"], model["gconst"]) for x in utts])
    lengths = [len(x) for x in utts]
    return ref.viterbi_batch(logb, lengths, model["log_start"], model["log_trans"], model["log_exit"], pen)


def _case_network(model, pen=0.0):
    from sapr_amd.connected import ConnectedNetwork
    return ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], pen, None, model["means"],
                            model["vars"], model["gconst"])


@pytest.mark.parametrize("case", ref.E2E_CASES)
def test_end_to_end_paths_equal_reference(case):
    """Paths and entries of EVERY utterance equal the reference (tests/test_connected_cpu.py guarantees the margins);
    score rtol 1e-12: a score is a sum of negative terms only, which leaves x10 over the emission bound."""
    from sapr_amd.connected import connected_decode
    seed, W, S, D, n = case
    model, utts, truth = ref.sample_case(seed, W, S, D, n)
    res = connected_decode(utts, _case_network(model))
    score, n_words, pw, ps, pe = _reference_decode(model, utts)
    rel = np.abs(res.score - score) / np.abs(score)
    print(f"end to end {case}: max relative score difference {rel.max():.3g}")
    assert np.array_equal(res.path_word, pw) and np.array_equal(res.path_state, ps)
    assert np.array_equal(res.path_entry, pe) and np.array_equal(res.n_words, n_words)
    assert rel.max() <= 1e-12
    assert sum(res.words(u) == truth[u] for u in range(n)) >= n // 2


def test_decoding_is_deterministic_and_independent_of_the_batch():
    from sapr_amd.connected import connected_decode
    seed, W, S, D, n = ref.E2E_CASES[0]
    model, utts, _ = ref.sample_case(seed, W, S, D, n)
    net = _case_network(model, pen=-5.0)
    a, b = connected_decode(utts, net), connected_decode(utts, net)
    for f in ("score", "n_words", "path_word", "path_state", "path_entry"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for u in (0, 7, n - 1):
        one = connected_decode([utts[u]], net)
        lo, hi = a.offsets[u], a.offsets[u + 1]
        assert one.score.tobytes() == a.score[u:u + 1].tobytes()
        assert np.array_equal(one.path_word, a.path_word[lo:hi]) and np.array_equal(one.path_state, a.path_state[lo:hi])
        assert np.array_equal(one.path_entry, a.path_entry[lo:hi]) and one.n_words[0] == a.n_words[u]


def _pickle_models(tmp_path, impl, models, names, n_iter=15):
    d = tmp_path / "trained_models" / impl
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_{impl}_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


def test_decoder_decode_connected(tmp_path):
    from sapr_amd.decoder import Decoder
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    seed, W, S, D, n = ref.DECODER_CASE
    model, utts, truth = ref.sample_case(seed, W, S, D, n, spherical=True)
    names = ["zero", "one", "two", "three"]
    models = []
    for w in range(W):
        ct = "spherical" if w % 2 else "diag"
        m = GaussianHMM(n_components=S, covariance_type=ct)
        m.startprob_, m.transmat_, m.means_ = model["startprob"][w], model["transmat"][w], model["means"][w]
        m._covars_ = model["vars"][w, :, 0].copy() if w % 2 else model["vars"][w]
        models.append(m)
    root = _pickle_models(tmp_path, "hmmlearn", models, names)
    dec = Decoder(models_dir=root, implementation="hmmlearn", n_iter=15)
    order = [names.index(w) for w in dec.vocab]                  # load order (glob) is the word order of the network
    sub = {k: v[order] for k, v in model.items()}
    for pen in (0.0, -30.0):
        got = dec.decode_connected([x.T for x in utts], word_penalty=pen)
        score, n_words, pw, ps, pe = _reference_decode(sub, utts, pen)
        offs = np.r_[0, np.cumsum([len(x) for x in utts])]
        for u, row in enumerate(got):
            lo, hi = offs[u], offs[u + 1]
            segs = ref.segments(pw[lo:hi], pe[lo:hi])
            assert row["words"] == [dec.vocab[w] for w, _, _ in segs]
            assert row["segments"] == [(dec.vocab[w], a, b) for w, a, b in segs]
            assert np.array_equal(row["state_sequence"], ps[lo:hi])
            assert abs(row["log_likelihood"] - score[u]) <= 1e-12 * abs(score[u])
            if pen == 0.0:
                assert row["words"] == [names[w] for w in truth[u]]
    # the three refusals name their reason
    full = GaussianHMM(n_components=S, covariance_type="full")
    root_full = _pickle_models(tmp_path / "f", "hmmlearn", models[:1] + [full], ["zero", "one"])
    with pytest.raises(ValueError, match="full"):
        Decoder(models_dir=root_full, implementation="hmmlearn").decode_connected([utts[0].T])
    for impl in ("custom", "gmmhmm"):
        other = _pickle_models(tmp_path / impl, impl, [{"placeholder": impl}], ["zero"])
        with pytest.raises(ValueError, match=impl):
            Decoder(models_dir=other, implementation=impl).decode_connected([utts[0].T])
