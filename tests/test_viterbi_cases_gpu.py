"""The Viterbi decoders on every instantiation and chain structure: viterbi_dense_kernel and viterbi_bidiag_kernel
(CAND = false through sapr_viterbi_diag_scores, CAND = true as the pruned decoder's second pass), both bounding passes
of sapr_viterbi_decode_pruned, the pack kernels' flags and the three back-trace kernels, on the inputs of
tests/_viterbi_cases.py (which see; tests/test_viterbi_cases_cpu.py checks the inputs and the oracles on the CPU).

The bar is the project's own and has no tolerance: float64 scores equal bit for bit, best words and state paths equal to
oracle/c_oracle.decode_batch with the same ``tie`` and ``sum_order``.

Which bounding pass a structure kind takes (asserted in test_bidiag_pruned: diag_pack_consts_kernel / gemm_entry /
diag_pack_gemm_consts_kernel decide it; every kind is inside the bound's domain, PACK_BOUND_OK, so all are pruned):
    start_spread, start_state3, absorbing, no_self_loop_48, head_and_tail, ties, long     matrix cores (PACK_GEMM_OK)
    no_self_loop (states 4 and 7: position 7 has no mask)                                 vector ALU
    two_chains (the -inf forward weight 5 -> 6 lies inside the reachable chain: no R_j)   vector ALU
``approx="valu"`` runs every kind on the vector ALU as well.

Non-finite frames (test_non_finite_frames_are_contained), what the kernels return for a touched utterance: see DESIGN §8.
"""
import numpy as np
import pytest

from tests import _fb_regimes as R
from tests import _viterbi_cases as V
from tests._synth import trained_like_models
from tests.test_viterbi_gpu import _assert_pruned_equals_full, _oracle, _ragged, _run_pruned

pytestmark = pytest.mark.gpu

TIES = ["high", "low"]
GEMM_OFF = ("no_self_loop", "two_chains")       # structure kinds whose pack must clear PACK_GEMM_OK
_DEVICE = {}


def _on_device(case):
    """(FeatureBatch, DiagModelPack) of a case, built once."""
    if id(case) not in _DEVICE:
        from sapr_amd import _lib
        from sapr_amd.trellis import DiagModelPack, FeatureBatch, kernel_dims, kernel_states
        batch = FeatureBatch.from_arrays(case.utts, layout="TD")
        pack = DiagModelPack.from_params(case.sp, case.A, case.mu, case.cv)
        assert pack.topology == (_lib.TOPO_BIDIAG if case.bidiag else _lib.TOPO_DENSE)
        assert (pack.S_model, pack.D_model) == (case.S, case.D) and pack.D == case.D == batch.D
        assert pack.S == kernel_states(case.S) and pack.S in (10, 18) and kernel_dims(case.D) == case.D
        assert pack.fast_div == 1
        _DEVICE[id(case)] = (case, batch, pack)
    return _DEVICE[id(case)][1:]


def _decode(case, tie, sum_order=1, fast_div=None, word_sel=None):
    import torch
    from sapr_amd import _lib
    from sapr_amd.trellis import viterbi_decode
    batch, pack = _on_device(case)
    res = viterbi_decode(batch, pack, tie=_lib.TIE_HIGH if tie == "high" else _lib.TIE_LOW, sum_order=sum_order,
                         word_sel=word_sel, fast_div=fast_div)
    torch.cuda.synchronize()
    return res


def _assert_equals_oracle(case, tie, sum_order, scores, best_word, best_score, path):
    osc, obw, opath = V.oracle(case, tie, sum_order)
    if scores is not None:
        np.testing.assert_array_equal(scores.cpu().numpy(), osc)
    np.testing.assert_array_equal(best_word.cpu().numpy(), obw)
    np.testing.assert_array_equal(best_score.cpu().numpy(), osc[np.arange(len(case.utts)), obw])
    np.testing.assert_array_equal(path.cpu().numpy(), opath)
    assert int(path.max()) < case.S


# ------------------------------------------------------------------------------------------------------
# dense route: viterbi_dense_kernel<D, S, TIE, SEQ, FASTDIV> and viterbi_backtrace_kernel<false>
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_div", [1, 0])
@pytest.mark.parametrize("sum_order", [1, 0])
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("fn_args", V.dense_cases(), ids=V.case_id)
def test_dense(fn_args, tie, sum_order, fast_div):
    """(every dense case has D = 13 or 39 unpadded — the padded ones pad S only — so both summation orders are exact)"""
    case = V.make(fn_args)
    assert not case.bidiag
    res = _decode(case, tie, sum_order, fast_div)
    _assert_equals_oracle(case, tie, sum_order, res.scores, res.best_word, res.best_score, res.path)


@pytest.mark.parametrize("fn_args", V.dense_cases(), ids=V.case_id)
def test_dense_word_sel_returns_each_models_own_path(fn_args):
    """The dense back-trace on a chosen model per utterance, against the numpy oracle (hmmlearn_oracle.decode itself on
    every fifth utterance of up to 300 frames, its row-at-a-time form on all of them)."""
    from oracle import hmmlearn_oracle as ho
    case = V.make(fn_args)
    n = len(case.utts)
    sel = (np.arange(n) + 1) % case.W
    tie = "low" if V.is_tie_case(case) else "high"       # (test_dense runs both rules on the best word's path)
    res = _decode(case, tie, word_sel=sel)
    bw, bs, path = res.best_word.cpu().numpy(), res.best_score.cpu().numpy(), res.path.cpu().numpy()
    np.testing.assert_array_equal(bw, sel)
    _, offs = V.packed(case)
    for u in range(n):
        w = sel[u]
        X = np.ascontiguousarray(case.utts[u].T).T
        lp, st = V.numpy_viterbi(X, case.sp[w], case.A[w], case.mu[w], case.cv[w], ties=(tie,))
        assert lp == bs[u], (u, w)
        np.testing.assert_array_equal(st[tie], path[offs[u]:offs[u + 1]])
        if u % 5 == 0 and X.shape[0] <= 300:
            lp2, st2 = ho.decode(X, case.sp[w], case.A[w], case.mu[w], case.cv[w], tie=tie)
            assert lp2 == bs[u]
            np.testing.assert_array_equal(st2, path[offs[u]:offs[u + 1]])


# ------------------------------------------------------------------------------------------------------
# bidiagonal route, every word: viterbi_bidiag_kernel<D, S, TIE, SEQ, FASTDIV, false>, viterbi_backtrace_kernel<true>
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sum_order", [1, 0])
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("fn_args", V.bidiag_cases(), ids=V.case_id)
def test_bidiag_all_vocabulary(fn_args, tie, sum_order):
    case = V.make(fn_args)
    assert case.bidiag
    res = _decode(case, tie, sum_order)
    _assert_equals_oracle(case, tie, sum_order, res.scores, res.best_word, res.best_score, res.path)


# the IEEE-division instantiations of the same kernel: the tie and long cases and the two most irregular structures
IEEE_CASES = [fa for fa in V.bidiag_cases() if fa[0] is not V.structure or fa[1][2] in ("head_and_tail", "two_chains")]


@pytest.mark.parametrize("sum_order", [1, 0])
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("fn_args", IEEE_CASES, ids=V.case_id)
def test_bidiag_all_vocabulary_ieee_division(fn_args, tie, sum_order):
    case = V.make(fn_args)
    res = _decode(case, tie, sum_order, fast_div=0)
    _assert_equals_oracle(case, tie, sum_order, res.scores, res.best_word, res.best_score, res.path)


# ------------------------------------------------------------------------------------------------------
# bidiagonal route, pruned: bounding pass (matrix cores or vector ALU), viterbi_select_kernel,
# viterbi_bidiag_kernel<.., CAND = true>, viterbi_backtrace_pruned_kernel
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("approx", ["auto", "valu"])
@pytest.mark.parametrize("sum_order", [1, 0])
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("fn_args", V.bidiag_cases(), ids=V.case_id)
def test_bidiag_pruned(fn_args, tie, sum_order, approx):
    from sapr_amd import _lib
    case = V.make(fn_args)
    full, dec, batch, pack = _run_pruned(case.utts, case.sp, case.A, case.mu, case.cv, tie=tie, sum_order=sum_order,
                                         approx=approx)
    assert pack.topology == _lib.TOPO_BIDIAG and pack.prunable and (pack.flags & _lib.PACK_BIDIAG)
    assert bool(pack.flags & _lib.PACK_GEMM_OK) == (case.name not in GEMM_OFF), (case, hex(pack.flags))
    kept = _assert_pruned_equals_full(full, dec)
    _assert_equals_oracle(case, tie, sum_order, None, dec.best_word, dec.best_score, dec.path)
    np.testing.assert_array_equal(full.scores.cpu().numpy(), V.oracle(case, tie, sum_order)[0])
    assert kept.cpu().numpy()[np.arange(len(case.utts)), dec.best_word.cpu().numpy()].all()    # the winner is kept
    print(f"{V.case_id(fn_args)} {tie} {sum_order} {approx}: kept {int(kept.sum())} of {kept.numel()} (utterance, word) pairs")


@pytest.mark.parametrize("sum_order,division", [(0, "fast"), (0, "ieee"), (1, "ieee")])
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("D,ns", V.SHAPES)
def test_pruned_decoder_pairwise_order_and_ieee_division(D, ns, tie, sum_order, division):
    """The CAND = true instantiations the canonical pruned test (sum_order = 1, fast division) leaves out, on the same
    kind of vocabulary: pruned against all-vocabulary against oracle."""
    from sapr_amd import _lib
    W = 11 if D == 13 else 4
    sp, A, mu, cv = trained_like_models(W, ns, D, seed=3)
    if division == "ieee":
        cv[1, 4, 7] = np.nextafter(32.0, 0.0)       # an all-ones significand: outside the fast division's domain
    utts = _ragged(200, D, seed=21)
    full, dec, batch, pack = _run_pruned(utts, sp, A, mu, cv, tie=tie, sum_order=sum_order)
    assert pack.fast_div == (division == "fast") and pack.prunable and (pack.flags & _lib.PACK_GEMM_OK)
    kept = _assert_pruned_equals_full(full, dec)
    osc, obw, opath = _oracle(utts, sp, A, mu, cv, tie, sum_order=sum_order)
    np.testing.assert_array_equal(full.scores.cpu().numpy(), osc)
    np.testing.assert_array_equal(dec.best_word.cpu().numpy(), obw)
    np.testing.assert_array_equal(dec.path.cpu().numpy(), opath)
    np.testing.assert_array_equal(dec.best_score.cpu().numpy(), osc[np.arange(len(utts)), obw])
    assert float(kept.double().mean()) < 0.6


# ------------------------------------------------------------------------------------------------------
# non-finite frames stay inside their utterance
# ------------------------------------------------------------------------------------------------------
def _bits(t):
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


@pytest.mark.parametrize("route", ["bidiag", "dense", "pruned-auto", "pruned-valu"])
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("D,ns", R.SHAPES)
def test_non_finite_frames_are_contained(D, ns, tie, route):
    """B' is B with a NaN, a +inf, a -inf (last frame) in three utterances of word 1 and a whole NaN frame in one of word
    2.  Every other utterance — among them the 63 lanes next to a touched one — keeps the bits of all W scores, of its best
    word and of its path rows.  A touched utterance: no finite score, pruned = all-vocabulary bit-wise, path entries inside
    0 .. S - 1.  (Not compared with an oracle: the C oracle and the numpy oracle disagree on a NaN frame.)"""
    import torch
    b, bp, touched = V.contained(D, ns, dense=(route == "dense"))
    n = len(b.utts)
    clean = np.asarray([u not in touched for u in range(n)])
    hit = np.asarray(sorted(touched))
    keep = torch.from_numpy(clean).cuda()
    rows = torch.from_numpy(np.repeat(clean, [x.shape[0] for x in b.utts])).cuda()
    assert clean.sum() == n - 4 and n > 256                  # more than one workgroup of utterances
    if route.startswith("pruned"):
        approx = route.split("-")[1]
        runs = [_run_pruned(c.utts, c.sp, c.A, c.mu, c.cv, tie=tie, approx=approx)[:2] for c in (b, bp)]
        for full, dec in runs:
            _assert_pruned_equals_full(full, dec)            # (NaN compares by bits)
        outs = [(full.scores, dec.best_word, dec.best_score, dec.path) for full, dec in runs]
    else:
        outs = []
        for c in (b, bp):
            r = _decode(c, tie)
            outs.append((r.scores, r.best_word, r.best_score, r.path))
    (sc0, bw0, bs0, p0), (sc1, bw1, bs1, p1) = outs
    _assert_equals_oracle(b, tie, 1, sc0, bw0, bs0, p0)      # the clean batch is right to begin with
    assert torch.equal(_bits(sc0[keep]), _bits(sc1[keep])), "scores of an untouched utterance changed"
    assert torch.equal(bw0[keep], bw1[keep]) and torch.equal(_bits(bs0[keep]), _bits(bs1[keep]))
    assert torch.equal(p0[rows], p1[rows]), "path rows of an untouched utterance changed"
    t_sc, t_bw, t_bs = sc1.cpu().numpy()[hit], bw1.cpu().numpy()[hit], bs1.cpu().numpy()[hit]
    t_path = p1[~rows].cpu().numpy()
    print(f"contained ({D}, {ns}) {route} {tie}: touched {touched}\n    scores {t_sc.tolist()}\n    best word {t_bw}, "
          f"best score {t_bs}, path entries {np.unique(t_path)}")
    assert not np.isfinite(t_sc).any() and not np.isfinite(t_bs).any()
    assert (t_bw == -1).all()                                # neither NaN nor -inf beats -inf: no word
    assert t_path.min() >= 0 and t_path.max() < b.S
