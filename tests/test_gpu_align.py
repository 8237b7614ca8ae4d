"""Rigid alignment to the baked field on the device (d3f_volume_align_*, csrc/align_kernels.hip; BakedField.normal_equations / align) against the
float64 restatement of tests/align_cases.py.

The accumulate: every entry of H, b and the cost within tol * A + slack of float64 -- A the same sum with absolute values at every product, slack
the coordinate terms of volume_cases, tol three times the worst ratio of the float32 port measured here (on the case and on its sibling whose
coordinates do not round), capped by align_cases.cap; counts exact; the padding of poisoned buffers untouched; a second run gives the same bytes.
The step: delta against numpy.linalg.solve, every transition against align_cases.step_ref.  The solve: CONVERGED on the two-sphere scene.

Mutants of the kernels and the assert that catches each:
  a corner pair or a face weight swapped in the derivative, wf / h dropped   test_accumulate_entry_by_entry (H, b)
  the group fold taking the wrong lane, a channel counted twice at a tail    the same test at C = 20 and 68, n = 17 and 65
  rows read for a point outside the band, or through the voxel index        the banded cases (NaN-poisoned invalid voxels)
  a workgroup's row at the wrong chunk, the fold skipping the odd chunks    n = 257 and 513; test_step_folds_the_chunks_in_order
  <= for < in the acceptance, lambda not clamped, a final state that moves  test_step_transitions_equal_the_restatement
"""
import ctypes

import numpy as np
import pytest
import torch

import align_cases as AC
import band_cases as BC
import volume_cases as VC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
POISON = -7.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def field_of(vol, dev):
    from d3fields_amd import BakedField
    sets = {k: torch.from_numpy(v).to(dev) for k, v in vol["sets"].items()}
    fills = {k: torch.from_numpy(f).to(dev) for k, f in vol["fills"].items() if f is not None}
    return BakedField.from_arrays(np.asarray(vol["origin"]).tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev),
                                  valid=torch.from_numpy(vol["valid"]).to(dev), fills=fills, **sets)


def pose_of(cases):
    return np.stack([np.concatenate([c["R"].reshape(9), c["t"]]) for c in cases]).astype(F)


def device_centroids(dev, p, w):
    I, n = p.shape[:2]
    out = torch.full((I + 1, 3), POISON, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().d3f_volume_align_centroid(_lib.ptr(p), _lib.ptr(w), I, n, _lib.ptr(out), _lib.current_stream_handle(dev)))
    assert (out[I] == POISON).all()
    return out[:I].contiguous()


def run_accumulate(field, cases, name="s0", wd=0.75, wf=1.25, outside=0.05, set_struct=None, use=("w", "targets", "dist_targets")):
    """one d3f_volume_align_accumulate through the C ABI on poisoned outputs one row too long -> (rows [I, 32], centroids [I, 3]) as NumPy;
    the instances of `cases` share a volume and a point count"""
    dev = field.device
    lib = _lib.load()
    I, n = len(cases), len(cases[0]["p"])
    p = torch.from_numpy(np.stack([c["p"] for c in cases])).to(dev)
    w = torch.from_numpy(np.stack([c["w"] for c in cases])).to(dev) if "w" in use else None
    tg = torch.from_numpy(np.stack([c["targets"] for c in cases])).to(dev) if name is not None and "targets" in use else None
    dt = torch.from_numpy(np.stack([c["dist_targets"] for c in cases])).to(dev) if "dist_targets" in use else None
    pose = torch.from_numpy(pose_of(cases)).to(dev)
    cen = device_centroids(dev, p, w)
    ws_bytes = lib.d3f_volume_align_workspace_bytes(I, n)
    results = []
    for _ in range(2):
        out = torch.full((I + 1, AC.ROW), POISON, dtype=torch.float64, device=dev)
        ws = torch.full((ws_bytes // 8 + AC.ROW,), POISON, dtype=torch.float64, device=dev)
        vol = field._volume()
        band = None if field.band is None else ctypes.byref(field._band_struct())
        sets = None if name is None else (set_struct if set_struct is not None else field._set_array([name]))
        _lib.check(lib.d3f_volume_align_accumulate(ctypes.byref(vol), band, sets, _lib.ptr(p), _lib.ptr(w), _lib.ptr(tg), _lib.ptr(dt), _lib.ptr(pose), _lib.ptr(cen),
                                                   None, I, n, wd, wf, outside, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
        torch.cuda.synchronize()
        out, ws = out.cpu().numpy(), ws.cpu().numpy()
        assert (out[I] == POISON).all() and (ws[ws_bytes // 8:] == POISON).all(), "the padding lost its poison"
        assert (out[:I, 30:] == 0).all() and (ws[:ws_bytes // 8].reshape(-1, AC.ROW)[:, 30:] == 0).all()
        results.append((out[:I], ws[:ws_bytes // 8]))
    assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes(), "two runs must agree byte for byte"
    return results[0][0], cen.cpu().numpy()


def check_rows(rows, cens, cases, mark, name, C, vec, wd=0.75, wf=1.25, outside=0.05, exact=None, use=("w", "targets", "dist_targets")):
    """every instance's row against float64 under tol * A + slack; -> the worst port ratio and the worst ratio of the device (for the record)"""
    def args(c, model):
        return (c["vol"], mark, name, c["p"], c["R"], c["t"], model, c["w"] if "w" in use else None, c["targets"] if name is not None else None,
                c["dist_targets"] if "dist_targets" in use else None, wd, wf, outside)

    port_worst = 0.0
    if exact is not None:
        m = AC.centroid(exact["p"], exact["w"])
        port_worst = max(AC.ratios(AC.accumulate32(*args(exact, m), vec=vec), AC.accumulate64(*args(exact, m)), slack=False))
    refs = []
    for i, c in enumerate(cases):
        want = AC.centroid(c["p"], c["w"] if "w" in use else None)
        assert np.all(np.abs(cens[i] - want) <= 2.0 ** -23 * np.abs(want)), "the device centroid is the float64 sum rounded once (one ulp for its other order)"
        ref = AC.accumulate64(*args(c, cens[i]))
        port_worst = max(port_worst, *AC.ratios(AC.accumulate32(*args(c, cens[i]), vec=vec), ref))
        refs.append(ref)
    tol = AC.tolerance(port_worst, C)
    dev_worst = 0.0
    for i, ref in enumerate(refs):
        H, b, cost, valid, in_band = AC.unpack_row(rows[i])
        assert (valid, in_band) == (ref["valid"], ref["in_band"]), (i, valid, in_band, ref["valid"], ref["in_band"])
        got = {"H": H, "b": b, "cost": cost}
        dev_worst = max(dev_worst, *AC.ratios(got, ref))
        assert np.all(np.abs(H - ref["H"]) <= tol * ref["A_H"] + ref["slack_H"]), (i, "H", dev_worst / AC.U, tol / AC.U)
        assert np.all(np.abs(b - ref["b"]) <= tol * ref["A_b"] + ref["slack_b"]), (i, "b", dev_worst / AC.U, tol / AC.U)
        assert abs(cost - ref["cost"]) <= tol * ref["A_cost"] + ref["slack_cost"], (i, "cost", dev_worst / AC.U, tol / AC.U)
    return port_worst, dev_worst


def instances(shape, C, n, I):
    """I instances in one volume with 10 % invalid voxels: plain, every image outside, specials (outside, NaN, zero weights)"""
    kinds = [dict(special=False), dict(special=False, away=True), dict(special=True)]
    return [AC.entry_case(shape, C, n, 3, 0.1, variant=v, **kinds[v]) for v in range(I)]


# ---- accumulate -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("banded", [False, True])
@pytest.mark.parametrize("C", AC.CHANNELS)
def test_accumulate_entry_by_entry(dev, C, banded):
    shape = "5x4x6"
    exact = AC.exact_case(shape, C, 65, 3, 0.1)
    vol = exact["vol"]
    f = field_of(vol, dev)
    mark = None
    if banded:
        band = AC.band_of(vol)
        mark = BC.mark(vol, band)
        f = f.to_band(float(band))
        assert np.array_equal(f.cell_band.cpu().numpy().astype(bool), mark["cell_band"]) and 0.2 < BC.kept_share(mark) < 0.9
    vec = C % 4 == 0
    # the sibling whose coordinates do not round: no slack, the device's own rounding against A alone
    rows, cens = run_accumulate(f, [exact])
    ref = AC.accumulate64(vol, mark, "s0", exact["p"], exact["R"], exact["t"], cens[0], exact["w"], exact["targets"], exact["dist_targets"], 0.75, 1.25, 0.05)
    port = AC.accumulate32(vol, mark, "s0", exact["p"], exact["R"], exact["t"], cens[0], exact["w"], exact["targets"], exact["dist_targets"], 0.75, 1.25, 0.05, vec=vec)
    H, b, cost, valid, in_band = AC.unpack_row(rows[0])
    port_exact, dev_exact = max(AC.ratios(port, ref, slack=False)), max(AC.ratios({"H": H, "b": b, "cost": cost}, ref, slack=False))
    print("C = %d %s, exact coordinates: worst ratio port %.3g, device %.3g (x 2^-24)" % (C, "banded" if banded else "dense", port_exact / AC.U, dev_exact / AC.U))
    assert (valid, in_band) == (ref["valid"], ref["in_band"]) and 0 < dev_exact <= AC.tolerance(port_exact, C)
    worst = [0.0, 0.0]
    counts = {"valid": 0, "out_of_band": 0, "weighted_invalid": 0}
    for n in AC.COUNTS:
        I = 3 if n in (17, 65, 257) else 1
        cases = instances(shape, C, n, I)
        assert all(c["vol"] is vol for c in cases)
        rows, cens = run_accumulate(f, cases)
        pw, dw = check_rows(rows, cens, cases, mark, "s0", C, vec, exact=exact)
        worst = [max(worst[0], pw), max(worst[1], dw)]
        counts["valid"] += int(rows[:, 28].sum())
        counts["out_of_band"] += int((rows[:, 28] - rows[:, 29]).sum())
        if I == 3:
            assert rows[1, 28] == 0 and not rows[1, :27].any() and rows[1, 27] > 0, "an instance with every image outside has a cost and nothing else"
            counts["weighted_invalid"] += n
    print("C = %d %s: worst ratio port %.3g, device %.3g, cap %.3g (x 2^-24)" % (C, "banded" if banded else "dense", worst[0] / AC.U, worst[1] / AC.U, AC.cap(C) / AC.U))
    assert counts["valid"] > 500 and counts["weighted_invalid"] > 0 and (counts["out_of_band"] > 100) == banded
    assert 0 < worst[0]


@pytest.mark.parametrize("C,n", [(3, 16), (68, 17)])
def test_accumulate_on_the_smallest_volume(dev, C, n):
    cases = [AC.entry_case("2x2x2", C, n, 1, 0.0, True)]
    f = field_of(cases[0]["vol"], dev)
    rows, cens = run_accumulate(f, cases)
    check_rows(rows, cens, cases, None, "s0", C, C % 4 == 0, exact=AC.exact_case("2x2x2", C, 33, 1))
    assert 0 < rows[0, 28] < n


@pytest.mark.parametrize("stride,offset,vec", [(23, 1, False), (24, 0, True), (24, 2, False), (20, 4, True)])
def test_accumulate_row_stride_and_alignment(dev, stride, offset, vec):
    """rows behind a stride larger than C and a base off 16-byte alignment: vectors only where the rule of d3f_volume_sample allows them"""
    C, n = 20, 65
    cases = instances("5x4x6", C, n, 3)
    vol = cases[0]["vol"]
    f = field_of(vol, dev)
    nvox = vol["dist"].size
    buf = torch.full((nvox * stride + offset + 8,), float("nan"), dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + nvox * stride].view(nvox, stride)
    view[:, :C] = torch.from_numpy(vol["sets"]["s0"].reshape(nvox, C)).to(dev)
    st = (_lib.VolumeSet * 1)(_lib.VolumeSet(view.data_ptr(), C, 0, stride, None))
    rows, cens = run_accumulate(f, cases, set_struct=st)          # (buf stays alive in this frame)
    check_rows(rows, cens, cases, None, "s0", C, vec, exact=AC.exact_case("5x4x6", C, 65, 3, 0.1))
    plain, _ = run_accumulate(f, cases)
    if vec:
        assert rows.tobytes() == plain.tobytes(), "the stride does not change the arithmetic"


def test_accumulate_without_a_set_and_without_optional_arrays(dev):
    C, n = 4, 65
    cases = instances("5x4x6", C, n, 3)
    f = field_of(cases[0]["vol"], dev)
    for banded in (False, True):
        g = f.to_band(float(AC.band_of(cases[0]["vol"]))) if banded else f
        mark = BC.mark(cases[0]["vol"], AC.band_of(cases[0]["vol"])) if banded else None
        rows, cens = run_accumulate(g, cases, name=None)
        check_rows(rows, cens, cases, mark, None, 1, False)
        plain = [dict(c, w=np.ones(n, F)) for c in cases]
        rows, cens = run_accumulate(g, plain, use=("targets",))
        check_rows(rows, cens, plain, mark, "s0", C, True, use=("targets",))
    # all weights zero: a row of zeros and a zero centroid
    none = [dict(cases[0], w=np.zeros(n, F))]
    rows, cens = run_accumulate(f, none)
    assert not rows.any() and not cens.any()
    # an empty band: no point is in it, the distance term is all there is
    empty = f.to_band(1e-12)
    assert empty.band_voxels.shape[0] == 0
    rows, cens = run_accumulate(empty, cases)
    ref, _ = run_accumulate(f, cases, name=None)
    assert rows[:, :28].tobytes() == ref[:, :28].tobytes() and not rows[:, 29].any() and np.array_equal(rows[:, 28], ref[:, 28])


def test_zero_residuals_give_exact_zeros_on_the_device(dev):
    """dist_weight = 0 and targets sampled by the field itself at the pose under test: the chain is d3f_volume_sample's, so r, b and the cost are 0"""
    c = AC.entry_case("5x4x6", 20, 257, 3, 0.1)
    f = field_of(c["vol"], dev)
    image = torch.from_numpy(AC.transform32(c["R"], c["t"], c["p"])).to(dev)
    sampled = f.eval(image)
    case = dict(c, targets=sampled["s0"].cpu().numpy())
    rows, _ = run_accumulate(f, [case], wd=0.0, outside=0.0)
    H, b, cost, valid, _ = AC.unpack_row(rows[0])
    assert valid == int((sampled["valid_mask"].cpu().numpy() & (c["w"] > 0)).sum()) > 50 and cost == 0.0 and not b.any() and np.linalg.eigvalsh(H).min() >= -1e-12 * np.abs(H).max()
    assert H[3:, 3:].any()


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
def run_step(dev, states, rows, it, iters, rot_tol, trans_tol, pose=None, skip=None, history=None, n=1):
    """one d3f_volume_align_step on I instances; rows [I, chunks, 32] is the workspace -> dict of NumPy arrays (state, out, pose, skip, history)"""
    lib = _lib.load()
    I = len(states)
    rows = np.asarray(rows, np.float64).reshape(I, -1, AC.ROW)
    st = torch.from_numpy(np.concatenate([np.asarray(states, np.float64), np.full((1, AC.STATE), POISON)])).to(dev)
    ws = torch.from_numpy(rows.copy()).to(dev)
    out = torch.full((I + 1, AC.ROW), POISON, dtype=torch.float64, device=dev)
    pose_t = torch.from_numpy(np.concatenate([np.full((I, 12), POISON, F) if pose is None else np.asarray(pose, F), np.full((1, 12), POISON, F)])).to(dev)
    skip_t = torch.from_numpy(np.concatenate([np.zeros(I, np.int32) if skip is None else np.asarray(skip, np.int32), np.full(1, -7, np.int32)])).to(dev)
    hist = np.full((I + 1, iters + 1), POISON) if history is None else np.concatenate([history, np.full((1, iters + 1), POISON)])
    hist_t = torch.from_numpy(hist).to(dev)
    assert lib.d3f_volume_align_workspace_bytes(I, n) == rows.nbytes
    _lib.check(lib.d3f_volume_align_step(_lib.ptr(st), _lib.ptr(ws), rows.nbytes, I, n, _lib.ptr(out), it, iters, rot_tol, trans_tol, _lib.ptr(pose_t), _lib.ptr(skip_t),
                                         _lib.ptr(hist_t), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    res = {"state": st.cpu().numpy(), "out": out.cpu().numpy(), "pose": pose_t.cpu().numpy(), "skip": skip_t.cpu().numpy(), "history": hist_t.cpu().numpy()}
    assert (res["state"][I] == POISON).all() and (res["out"][I] == POISON).all() and (res["pose"][I] == POISON).all() and res["skip"][I] == -7 and (res["history"][I] == POISON).all()
    assert (np.delete(res["history"][:I], it, axis=1) == hist[:I][:, [k for k in range(iters + 1) if k != it]]).all(), "one history entry per call"
    return {k: v[:I] for k, v in res.items()}


def crafted_systems(count, seed=0):
    """symmetric positive definite H with condition numbers up to 1e6, b, as rows"""
    rng = np.random.default_rng(seed)
    rows, Hs = [], []
    for i in range(count):
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        H = Q @ np.diag(10.0 ** np.linspace(0, -6 * i / max(count - 1, 1), 6)) @ Q.T * 10.0 ** rng.uniform(-3, 3)
        H = AC._mirror(H)
        row = np.zeros(AC.ROW)
        row[:21], row[21:27], row[27], row[28], row[29] = H[AC.TRIU], rng.standard_normal(6) * np.sqrt(np.diag(H)), 1.0 + i, 10, 7
        rows.append(row)
        Hs.append(H)
    return np.stack(rows), Hs


def test_step_solves_the_damped_system(dev):
    rows, Hs = crafted_systems(12)
    states = [AC.new_state(AC.rotation((1, 2, 3), 0.4), (0.1, -0.2, 0.3), (0.05, 0.02, -0.04)) for _ in rows]
    res = run_step(dev, states, rows, 0, 5, 1e-5, 1e-5)
    assert np.array_equal(res["out"], rows), "one chunk: the folded row is the row"
    for i, H in enumerate(Hs):
        D = np.diag(np.maximum(np.diag(H), 1e-9 * np.diag(H).max()))
        A = H + AC.LAMBDA0 * D
        cond = np.linalg.cond(A)
        assert cond <= 1.1e6
        want = np.linalg.solve(A, -rows[i, 21:27])
        delta = res["state"][i, AC.S_DELTA:AC.S_DELTA + 6]
        assert np.linalg.norm(delta - want) <= 100 * cond * 2.0 ** -53 * np.linalg.norm(want), (i, cond)
        ref = states[i].copy()
        hist, pose, skip = AC.step_ref(ref, rows[i], 0, 5, 1e-5, 1e-5)
        assert np.allclose(res["state"][i], ref, rtol=1e-9, atol=1e-7) and np.array_equal(res["state"][i, 27:33], ref[27:33])
        assert np.allclose(res["pose"][i], pose, rtol=0, atol=2e-7 * (1 + np.abs(pose).max())) and res["skip"][i] == skip == 0 and res["history"][i, 0] == hist
        R = res["pose"][i, :9].reshape(3, 3).astype(np.float64)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and abs(np.linalg.det(R) - 1) < 1e-6


def test_step_folds_the_chunks_in_order(dev):
    """even chunks in one half of the wave, odd chunks in the other, each in ascending order, then even + odd"""
    rng = np.random.default_rng(4)
    chunks = 5
    parts = rng.standard_normal((2, chunks, AC.ROW)) * 10.0 ** rng.uniform(-8, 8, (2, chunks, 1))
    parts[:, :, :21] = np.eye(6)[AC.TRIU] * (1 + np.abs(parts[:, :, :21]))
    states = [AC.new_state(np.eye(3), np.zeros(3), np.zeros(3)) for _ in range(2)]
    res = run_step(dev, states, parts, 0, 2, 1e-5, 1e-5, n=256 * (chunks - 1) + 1)
    want = ((parts[:, 0] + parts[:, 2]) + parts[:, 4]) + (parts[:, 1] + parts[:, 3])
    assert res["out"].tobytes() == want.tobytes()


def test_step_transitions_equal_the_restatement(dev):
    """planted cost sequences, one per instance: accepted steps down to the clamp of lambda, an equal cost, NaN costs and rises up to STALLED,
    convergence on a small step that was accepted or proposed right after an acceptance, NO_GRADIENT, FAILED, RUNNING at the end; status, lambda, steps, cost, skip and history equal the
    restatement exactly at every call, and a final instance never changes again"""
    iters = 26
    H = np.diag([4.0, 3.0, 2.0, 5.0, 6.0, 7.0])
    base = np.zeros(AC.ROW)
    base[:21], base[21:27], base[28], base[29] = H[AC.TRIU], 1e-3 * np.arange(1, 7), 9, 9
    falling = [5.0, 4.0, 3.0, 2.5, 2.0, 1.5, 1.0, 0.9, 0.8, 0.8] + [float("nan"), 0.8] * 8 + [float("nan")]
    plans = {
        "falling, equal, then stalled": (falling, base, 0.0, 0.0),
        "always falling": ([100.0 * 0.5 ** k for k in range(iters + 1)], base, 0.0, 0.0),
        "small after rejections, converged once accepted": ([1.0, 1.0, 2.0, 1.0, 0.5] + [0.4] * 22, base, 1e-3, 1e-3),
        "converged on the step proposed at the start": ([1.0] * (iters + 1), base, 1e-2, 1e-2),
        "rotation above its tolerance": ([1.0, 0.9, 0.8] + [0.8] * 24, base, 1e-9, 1.0),
        "no gradient": ([3.0] * (iters + 1), np.where(np.arange(AC.ROW) < 27, 0.0, base), 1e-5, 1e-5),
        "not finite": ([3.0] * (iters + 1), np.where(np.arange(AC.ROW) == 1, np.inf, base), 1e-5, 1e-5),
        "negative pivot": ([3.0] * (iters + 1), np.where(np.arange(AC.ROW) == 1, 100.0, base), 1e-5, 1e-5),
    }
    finals = {}
    for name, (costs, row0, rot_tol, trans_tol) in plans.items():
        assert len(costs) == iters + 1, name
        ref = AC.new_state(AC.rotation((0, 0, 1), 0.1), (0.01, 0.02, 0.03), (0.1, 0.0, -0.1))
        state = ref[None].copy()
        pose, skip, history = None, None, None
        ref_history = np.full(iters + 1, POISON)
        for it, cost in enumerate(costs):
            row = row0.copy()
            row[27] = cost
            before = state.copy()
            res = run_step(dev, state, row[None, None], it, iters, rot_tol, trans_tol, pose, skip, history)
            ref_history[it], ref_pose, ref_skip = AC.step_ref(ref, row, it, iters, rot_tol, trans_tol)
            state, pose, skip, history = res["state"], res["pose"], res["skip"], res["history"]
            assert np.array_equal(state[0, 27:33], ref[27:33]), (name, it, state[0, 27:33], ref[27:33])          # lambda, cost, status, steps, counts
            assert history[0, it] == ref_history[it] and skip[0] == ref_skip, (name, it)
            assert np.allclose(state[0], ref, rtol=1e-9, atol=2e-6), (name, it)          # (poses: float32 values, a last-place difference of sin may move one)
            if int(before[0, AC.S_STATUS]) != AC.RUNNING:
                assert state.tobytes() == before.tobytes(), (name, it, "a final state moved")
            else:
                assert np.allclose(pose[0], ref_pose, rtol=0, atol=2e-6 * (1 + np.abs(ref_pose).max())), (name, it)
        finals[name] = (int(state[0, AC.S_STATUS]), int(state[0, AC.S_STEPS]), state[0, AC.S_LAMBDA])
    print(finals)
    assert finals["falling, equal, then stalled"][:2] == (AC.STALLED, 8) and finals["falling, equal, then stalled"][2] == 1e6
    assert finals["always falling"] == (AC.RUNNING, iters, 1e-9)
    assert finals["small after rejections, converged once accepted"] == (AC.CONVERGED, 1, 0.1)
    assert finals["converged on the step proposed at the start"] == (AC.CONVERGED, 0, 1e-3)
    assert finals["rotation above its tolerance"][0] == AC.STALLED and finals["rotation above its tolerance"][1] == 2
    assert finals["no gradient"][:2] == (AC.NO_GRADIENT, 0) and finals["not finite"][:2] == (AC.FAILED, 0) and finals["negative pivot"][:2] == (AC.FAILED, 0)


# ---- the solve ------------------------------------------------------------------------------------------------------------------------------
def scene_inputs(dev, starts, banded):
    s = AC.scene()
    f = field_of(s["vol"], dev)
    if banded:
        f = f.to_band(AC.SCENE_BAND_STEPS * VC.STEP)
    I = len(starts)
    poses = [AC.scene_start(*st) for st in starts]
    rot = torch.from_numpy(np.stack([R.T for R, _ in poses])).to(dev)             # the row-vector convention: the transpose of the kernels' R
    trans = torch.from_numpy(np.stack([t for _, t in poses])).to(dev)
    pts = torch.from_numpy(np.repeat(s["p"][None], I, 0)).to(dev)
    tg = torch.from_numpy(np.repeat(s["targets"][None], I, 0)).to(dev)
    return f, pts, tg, rot.contiguous(), trans


@pytest.mark.parametrize("banded", [False, True])
def test_align_converges_on_the_scene(dev, banded):
    from d3fields_amd.rigid import rigid_transform
    f, pts, tg, rot, trans = scene_inputs(dev, AC.STARTS, banded)
    fit = f.align(pts, "feat", tg, rot=rot, trans=trans, iters=20)
    assert set(fit) == {"rot", "trans", "points", "cost", "valid", "status", "steps", "history"} and not any(v.requires_grad for v in fit.values())
    hist = fit["history"].cpu().numpy()
    errors = [AC.point_error_voxels(x) for x in fit["points"].cpu().numpy()]
    print("banded" if banded else "dense", "status", fit["status"].tolist(), "steps", fit["steps"].tolist(), "errors (voxels)", np.round(errors, 5), "cost", hist[:, 0], "->", hist[:, -1])
    assert fit["status"].tolist() == [AC.CONVERGED] * len(AC.STARTS)
    assert hist.shape == (len(AC.STARTS), 21) and np.all(np.diff(hist, axis=1) <= 0) and np.array_equal(hist[:, -1], fit["cost"].cpu().numpy())
    assert max(errors) < 0.1
    assert fit["valid"].tolist() == [225] * len(AC.STARTS) and all(1 <= k <= 20 for k in fit["steps"].tolist())
    # rigid_transform reproduces the points within the rounding of the two chains: each three products and three sums of magnitude |p| |R| + |t|
    again = rigid_transform(pts, fit["rot"], fit["trans"])
    scale = (pts.abs() @ fit["rot"].abs() + fit["trans"].abs()[:, None, :])
    assert torch.all((again - fit["points"]).abs() <= 8 * 2.0 ** -24 * scale)
    # a frozen instance: more iterations change nothing
    longer = f.align(pts, "feat", tg, rot=rot, trans=trans, iters=27)
    for k in ("rot", "trans", "points", "cost", "valid", "status", "steps"):
        assert torch.equal(fit[k], longer[k]), k
    assert torch.equal(longer["history"][:, :21], fit["history"]) and torch.equal(longer["history"][:, 21:], fit["cost"][:, None].expand(-1, 7))
    # the restatement ends at the same place (not the same bytes: its sums are NumPy's)
    s = AC.scene()
    mark = BC.mark(s["vol"], AC.SCENE_BAND_STEPS * VC.STEP) if banded else None
    ref = AC.align_ref(s["vol"], mark, "feat", s["p"], *AC.scene_start(*AC.STARTS[1]), targets=s["targets"])
    assert ref["status"] == AC.CONVERGED
    assert np.abs(fit["points"][1].cpu().numpy() - ref["points"]).max() < 1e-3 * VC.STEP and abs(ref["cost"] - hist[1, -1]) <= 1e-6 * hist[1, 0]


def test_many_starts_are_many_instances(dev):
    """64 starts around one truth as 64 instances give what 64 separate calls give, byte for byte"""
    rng = np.random.default_rng(64)
    starts = [(float(rng.uniform(1, 10)), float(rng.uniform(0.2, 2.5)), 1000 + k) for k in range(64)]
    f, pts, tg, rot, trans = scene_inputs(dev, starts, False)
    fit = f.align(pts, "feat", tg, rot=rot, trans=trans, iters=8)
    assert (fit["status"] == AC.CONVERGED).sum().item() >= 48
    errors = np.array([AC.point_error_voxels(x) for x in fit["points"].cpu().numpy()])
    assert errors[(fit["status"] == AC.CONVERGED).cpu().numpy()].max() < 0.1
    best = int(torch.argmin(fit["cost"]))
    assert errors[best] < 0.1
    single = [f.align(pts[k:k + 1], "feat", tg[k:k + 1], rot=rot[k:k + 1], trans=trans[k:k + 1], iters=8) for k in range(64)]
    for key in fit:
        alone = torch.cat([s[key] for s in single], dim=0)
        assert alone.cpu().numpy().tobytes() == fit[key].cpu().numpy().tobytes(), key


# ---- the public layer ---------------------------------------------------------------------------------------------------------------------
def test_normal_equations_is_the_accumulate(dev):
    cases = instances("5x4x6", 20, 65, 3)
    f = field_of(cases[0]["vol"], dev)
    rows, _ = run_accumulate(f, cases, outside=0.05)
    t = lambda key: torch.from_numpy(np.stack([c[key] for c in cases])).to(dev)
    rot = torch.from_numpy(np.stack([c["R"].T for c in cases])).to(dev).contiguous()
    ne = f.normal_equations(t("p"), rot, t("t"), name="s0", targets=t("targets"), dist_targets=t("dist_targets"), weights=t("w"), dist_weight=0.75, feat_weight=1.25,
                            outside=0.05)
    assert ne["H"].dtype == torch.float64 and tuple(ne["H"].shape) == (3, 6, 6) and torch.equal(ne["H"], ne["H"].transpose(1, 2))
    for i in range(3):
        H, b, cost, valid, in_band = AC.unpack_row(rows[i])
        assert np.array_equal(ne["H"][i].cpu().numpy(), H) and np.array_equal(ne["b"][i].cpu().numpy(), b) and ne["cost"][i].item() == cost
        assert (ne["valid"][i].item(), ne["in_band"][i].item()) == (valid, in_band)
    assert ne["valid"].dtype == ne["in_band"].dtype == torch.int32 and not any(v.requires_grad for v in ne.values())
    # the default of `outside` is 4 * step * dist_weight
    a = f.normal_equations(t("p"), rot, t("t"), dist_weight=0.5)
    b = f.normal_equations(t("p"), rot, t("t"), dist_weight=0.5, outside=4 * f.step * 0.5)
    assert torch.equal(a["cost"], b["cost"]) and a["cost"][1].item() > 0 and a["valid"][1].item() == 0


def test_public_layer_errors_and_empty_problems(dev):
    s = AC.scene()
    f = field_of(s["vol"], dev)
    pts = torch.from_numpy(s["p"][None]).to(dev)
    tg = torch.from_numpy(s["targets"][None]).to(dev)
    eye = torch.eye(3, device=dev)[None]
    zero = torch.zeros((1, 3), device=dev)
    for call in (lambda **kw: f.align(kw.pop("points", pts), **kw), lambda **kw: f.normal_equations(kw.pop("points", pts), kw.pop("rot", eye), kw.pop("trans", zero), **kw)):
        with pytest.raises(ValueError):
            call(points=pts[0])
        with pytest.raises(ValueError):
            call(name="feat", targets=tg[:, :10])
        with pytest.raises(ValueError):
            call(name="feat")
        with pytest.raises(ValueError):
            call(targets=tg)
        with pytest.raises(ValueError):
            call(weights=torch.ones((1, 224), device=dev))
        with pytest.raises(ValueError):
            call(dist_weight=-1.0)
        with pytest.raises(ValueError):
            call(rot=torch.eye(3, device=dev))
        with pytest.raises(TypeError):
            call(points=pts.double())
        with pytest.raises(TypeError):
            call(name="feat", targets=tg.half())
        with pytest.raises(KeyError):
            call(name="nope", targets=tg)
        with pytest.raises(RuntimeError):
            call(points=pts.cpu())
        with pytest.raises(RuntimeError):
            call(name="feat", targets=tg.cpu())
    with pytest.raises(ValueError):
        f.align(pts, iters=-1)
    with pytest.raises(ValueError):
        f.align(pts, rot_tol=float("nan"))
    # I == 0 and n == 0: nothing is launched, the shapes are those of the request
    fit = f.align(pts[:0], "feat", tg[:0], iters=3)
    assert tuple(fit["rot"].shape) == (0, 3, 3) and tuple(fit["points"].shape) == (0, 225, 3) and tuple(fit["history"].shape) == (0, 4) and fit["status"].numel() == 0
    fit = f.align(pts[:, :0], "feat", tg[:, :0], rot=eye, trans=zero + 0.5, iters=3)
    assert fit["status"].tolist() == [AC.NO_GRADIENT] and torch.equal(fit["rot"], eye) and torch.equal(fit["trans"], zero + 0.5) and tuple(fit["points"].shape) == (1, 0, 3)
    assert fit["cost"].tolist() == [0.0] and fit["valid"].tolist() == [0] and fit["steps"].tolist() == [0]
    ne = f.normal_equations(pts[:0], eye[:0], zero[:0])
    assert tuple(ne["H"].shape) == (0, 6, 6) and tuple(ne["b"].shape) == (0, 6)
    ne = f.normal_equations(pts[:, :0], eye, zero)
    assert not ne["H"].any() and ne["valid"].tolist() == [0]
    # every point outside: NO_GRADIENT, the pose is the start's, the cost is the penalty
    fit = f.align(pts, "feat", tg, trans=zero + 10.0, outside=0.5)
    assert fit["status"].tolist() == [AC.NO_GRADIENT] and torch.equal(fit["trans"], zero + 10.0) and fit["cost"].tolist() == [225 * 0.25] and fit["valid"].tolist() == [0]
    # RUNNING: the iterations ran out
    R, t = AC.scene_start(10.0, 2.5, 1)
    fit = f.align(pts, "feat", tg, rot=torch.from_numpy(R.T.copy()).to(dev)[None], trans=torch.from_numpy(t).to(dev)[None], iters=1)
    assert fit["status"].tolist() == [AC.RUNNING] and fit["steps"].tolist() == [1] and fit["history"][0, 1] < fit["history"][0, 0]
