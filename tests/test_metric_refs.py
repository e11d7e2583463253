"""CPU: the float64 definition of tests/metric_cases.py IS the Inter and Center terms of the reference's utils/loss.py:43-79, its
bars hold a float32 evaluation of the same statements and reject the likely mistakes, and the case table holds every condition the
GPU test relies on -- what keeps tests/test_gpu_metric_terms.py from hiding a failure.

The reference's statements (utils/loss.py:46-79 there), restated below with torch operators in this test's own names (its file
is not imported and none of its text is taken over): per image, `unique` of the flat labels with counts and the sum of the counts
(every pixel) as the divisor; for every class present but ignore_index the flat pixel indices, `index_select` of the pixel-major
logits and of the features, the mean over the selected features, the sum of their squared deviations over the divisor into
Center, (the sum of the selected logits - the sum of their own-class column) over the divisor into Inter;
(beta Inter + gamma Center) / n at the end.  One departure: the features of an image are taken as [H W, C] before the
`index_select`; the reference passes [H, W, C] and selects along H with flat indices, which raises as soon as an index >= H.
"""
import numpy as np
import pytest
import torch

import metric_cases as MC

F64 = np.float64
NAMES = list(MC.CASES)


def class_rows(labels_flat, skip):
    """-> (classes present but `skip`, number of labelled pixels): `unique` with counts, as the reference takes them per image"""
    present, how_many = torch.unique(labels_flat, return_counts=True)
    return [int(k) for k in present.tolist() if int(k) != skip], int(how_many.sum())


def torch_statements(lg, f, y, ignore_index, beta, gamma, dtype, gout=1.0):
    """the reference's loop (utils/loss.py:46-79 there) in this test's own words
    -> (term, Inter per image, Center per image, d term / d logits, d term / d features), the gradients by autograd"""
    L = torch.from_numpy(np.array(lg)).to(dtype).requires_grad_(True)
    F = torch.from_numpy(np.array(f)).to(dtype).requires_grad_(True)
    Y = torch.from_numpy(np.array(y))
    batch, K = L.shape[0], L.shape[1]
    per_image = []
    for img in range(batch):
        flat_y = Y[img].reshape(-1)
        pixel_logits = L[img].reshape(K, -1).t()                         # [H W, K]
        pixel_feats = F[img].reshape(flat_y.numel(), -1)                 # [H W, C]: flat, where the reference keeps [H, W, C]
        classes, pixels = class_rows(flat_y, ignore_index)
        push = torch.zeros((), dtype=dtype)                               # the other classes' logits
        spread = torch.zeros((), dtype=dtype)                             # the squared deviations from the class mean
        for k in classes:
            rows = (flat_y == k).nonzero().squeeze(1)
            lk = pixel_logits.index_select(0, rows)
            fk = pixel_feats.index_select(0, rows)
            dev = fk - fk.mean(dim=0)
            spread = spread + dev.pow(2).sum() / pixels
            push = push + (lk.sum() - lk[:, k].sum()) / pixels
        per_image.append((push, spread))
    inter_total = sum(p for p, _ in per_image)
    center_total = sum(c for _, c in per_image)
    term = (beta * inter_total + gamma * center_total) / batch
    (gout * term).backward()
    return (term.item(), np.array([p.item() for p, _ in per_image]), np.array([c.item() for _, c in per_image]),
            L.grad.double().numpy(), F.grad.double().numpy())


def weights(case):
    return float(np.float32(case["beta"])), float(np.float32(case["gamma"]))


@pytest.mark.parametrize("name", NAMES)
def test_definition_is_the_references_statements_in_float64(name):
    case = MC.CASES[name]
    lg, f, y = MC.inputs(name)
    beta, gamma = weights(case)
    ref = MC.metric_ref(lg, f, y, case["ignore"], beta, gamma, gout=case["gout"])
    term, inter, center, gl, gf = torch_statements(lg, f, y, case["ignore"], beta, gamma, torch.float64, gout=case["gout"])
    rel = lambda a, b: np.abs(a - b).max() / max(1e-300, np.abs(b).max()) if np.abs(b).max() > 0 else np.abs(a).max()
    assert rel(np.array(term), np.array(ref["term"])) <= 1e-12
    assert rel(inter, ref["inter"]) <= 1e-12 and rel(center, ref["center"]) <= 1e-12
    # autograd goes through the mean: the definition's gradient has no such part because it cancels
    assert rel(gl, ref["gl"]) <= 1e-12 and rel(gf, ref["gf"]) <= 1e-12
    assert (gl[ref["gl"] == 0] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_float32_statements_lie_inside_the_bars(name):
    """the bars of the kernels' launch shapes hold torch's float32 evaluation too: its sums run in another order but no deeper.
    What it rounds in float32 and the kernels do in double is added: the per-image quotient, the accumulators, the weights and
    the division by n (8 eps of the magnitudes on the term, 4 eps on a per-image value and on a gradient element)"""
    case = MC.CASES[name]
    lg, f, y = MC.inputs(name)
    beta, gamma = weights(case)
    ref = MC.metric_ref(lg, f, y, case["ignore"], beta, gamma, gout=case["gout"], chain="kernel")
    term, inter, center, gl, gf = torch_statements(lg, f, y, case["ignore"], beta, gamma, torch.float32, gout=case["gout"])
    n = lg.shape[0]
    slack = 8 * MC.EPS32 * (abs(beta) * np.abs(ref["inter"]).sum() + abs(gamma) * ref["center"].sum()) / n
    e_gf = np.abs(gf - ref["gf"])
    # torch rounds the weight chain (gout, / n, / the pixel count, 2 x) four times more
    gf_bar = ref["gf_bar"] + 4 * MC.EPS32 * np.abs(ref["gf"])
    gl_bar = ref["gl_bar"] + 4 * MC.EPS32 * np.abs(ref["gl"])
    print("MEASURE %s float32 torch: term err %.3e bar %.3e | Inter_i err/bar %.3f | Center_i err/bar %.3f | gF err/bar %.3f"
          % (name, abs(term - ref["term"]), ref["term_bar"] + slack,
             (np.abs(inter - ref["inter"]) / np.maximum(ref["inter_bar"] + 4 * MC.EPS32 * np.abs(ref["inter"]), 1e-300)).max(),
             (np.abs(center - ref["center"]) / np.maximum(ref["center_bar"] + 4 * MC.EPS32 * ref["center"], 1e-300)).max(),
             (e_gf / np.maximum(gf_bar, 1e-300)).max()))
    assert abs(term - ref["term"]) <= ref["term_bar"] + slack
    assert (np.abs(inter - ref["inter"]) <= ref["inter_bar"] + 4 * MC.EPS32 * np.abs(ref["inter"])).all()
    assert (np.abs(center - ref["center"]) <= ref["center_bar"] + 4 * MC.EPS32 * ref["center"]).all()
    assert (np.abs(gl - ref["gl"]) <= gl_bar).all() and (gl[ref["gl"] == 0] == 0).all()
    assert (e_gf <= gf_bar).all()
    assert (gf[~ref["valid"]] == 0).all()


def outside(ref, mut):
    """-> (largest distance of a mutant from the definition in bars, over the elements whose bar is not 0; number of elements
    with a zero bar, which must be exactly right, that it changes).  The two are not mixed: a ratio to a zero bar has no meaning."""
    worst, exact_broken = 0.0, 0
    for key, bar in (("term", "term_bar"), ("inter", "inter_bar"), ("center", "center_bar"), ("gl", "gl_bar"), ("gf", "gf_bar"),
                     ("means", "means_bar")):
        d = np.abs(np.asarray(mut[key]) - np.asarray(ref[key])).reshape(-1)
        b = np.asarray(ref[bar], dtype=F64).reshape(-1)
        pos = b > 0
        worst = max(worst, float((d[pos] / b[pos]).max(initial=0.0)))
        exact_broken += int((d[~pos] != 0).sum())
    return worst, exact_broken


@pytest.mark.parametrize("what", list(MC.MUTANTS))
def test_bars_reject_the_mutants(what):
    """each likely mistake moves an element with a non-zero bar by at least 100 bars, on the case named for it; the elements with
    a zero bar that it changes are counted apart"""
    name = MC.MUTANTS[what]
    case = MC.CASES[name]
    lg, f, y = MC.inputs(name)
    ref = MC.reference(name)
    mut = MC.metric_ref(lg, f, y, case["ignore"], case["beta"], case["gamma"], gout=case["gout"], mutant=what)
    off, exact_broken = outside(ref, mut)
    print("MEASURE %s on %s: %.0f bars away on the elements with a bar, %d exact elements changed" % (what, name, off, exact_broken))
    assert off >= 100
    if what in ("own class in Inter", "ignored pixels counted"):
        assert exact_broken > 0                                          # the own-class plane / the ignored pixels stop being 0
    if what.startswith("Center as"):
        # the cancelling form loses the centre term itself on the offset case: off by more than a tenth of its value
        assert (np.abs(mut["center"] - ref["center"]) > 0.1 * ref["center"]).all()
        assert (np.abs(mut["center"] - ref["center"]) > 100 * ref["center_bar"]).all()


def test_the_case_table_holds_every_condition():
    C = MC.CASES
    shapes = {(c["H"], c["W"]) for c in C.values()}
    assert shapes == {(1, 1), (3, 5), (17, 23), (96, 160)}
    assert {c["B"] for c in C.values()} == {1, 3}
    assert {(c["K"], c["C"]) for c in C.values()} == {(2, 1), (16, 16), (17, 17), (32, 32), (16, 5)}
    assert {c["ignore"] for c in C.values()} == {255, -1}
    assert {c["feats"] for c in C.values()} == {"trained", "offset", "constant"}
    assert any(c["beta"] != 0 and c["gamma"] == 0 for c in C.values()) and any(c["beta"] == 0 and c["gamma"] != 0 for c in C.values())
    assert any(c["beta"] != 0 and c["gamma"] != 0 for c in C.values()) and any(c["gout"] != 1 for c in C.values())
    assert any((c["H"] * c["W"] * c["C"]) % 4 for c in C.values()) and any((c["H"] * c["W"] * c["C"]) % 4 == 0 for c in C.values())
    # several workgroups per image in every launch: more than 256 groups of four floats, of four pixels, and pixel steps
    d = MC.chain_depths(3, 96, 160, 16, 16)
    assert 96 * 160 * 16 // 4 > 256 and 96 * 160 // 4 > 256 and d[0] >= 1
    for name, c in C.items():
        lg, f, y = MC.inputs(name)
        ign = (y == c["ignore"])
        assert lg.dtype == np.float32 and f.dtype == np.float32 and y.dtype == np.int64
        assert ((y >= 0) & (y < c["K"]))[~ign].all()
        if c["labels"] == "mix" and y[0].size > 100:
            assert 0.10 <= ign.mean() <= 0.20, name
        if c["labels"] == "edges":
            ref = MC.reference(name)
            assert ref["counts"][0, 1] == 1 and ref["counts"][0, 0] == 0 and ref["counts"][2, 0] > 0    # one pixel; absent / present
            assert ign[1].all() and ref["counts"][1].sum() == 0                                          # an image entirely ignored
            assert (ref["counts"][2] > 0).sum() == 1                                                     # an image of a single class
            assert ref["inter"][1] == 0 and ref["center"][1] == 0 and not ref["gf"][1].any() and not ref["gl"][1].any()
            one = (y[0] == 1)
            assert one.sum() == 1 and not ref["gf"][0][one].any() and not ref["gf_bar"][0][one].any()
        if c["feats"] == "offset":
            assert abs(f.mean() - 50) < 0.01 and 0.005 < f.std() < 0.02
        if c["feats"] == "constant":
            ref = MC.reference(name)
            assert not ref["center"].any() and not ref["center_bar"].any() and not ref["gf"].any() and not ref["gf_bar"].any()
            assert not ref["means_bar"].any() and ref["inter"].all()
    # ignored pixels and own-class logits have a zero bar everywhere
    ref = MC.reference("96x160")
    lg, f, y = MC.inputs("96x160")
    assert not ref["gf_bar"][y == 255].any() and not ref["gl_bar"].transpose(0, 2, 3, 1)[y == 255].any()
    own = np.arange(16)[None, :, None, None] == y[:, None]
    assert not ref["gl_bar"][own].any() and ref["gl_bar"][~own & (y != 255)[:, None]].all()
