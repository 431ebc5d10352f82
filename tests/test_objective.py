"""The closed-form training objective on the GPU (ocffm_problem_objective,
ocffm_problem_solve_ex, train --objective / --tol) against the
oracle's func() and a dense numpy evaluation of the same state.

Bounds: fp64 within 1e-12 relative of the dense evaluation of the same state
and of func() at init, within the project's 1e-9 of the oracle after epochs;
fp32 within 1e-3 (the project's fp32 objective contract) of the fp64
evaluation of the downloaded fp32 state.  The measured errors are printed.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import objective_ref as R
import ocffm
import oracle_lib as O
import synth
from test_gpu_parity import TRAIN, fp64_tol, pair, rel, state_names

pytestmark = pytest.mark.gpu

TERMS = ("pos", "on_pos", "all", "reg")


def shape(name):
    if name == "tiny":
        return synth.tiny()
    k, fu, fv = {"k5": (5, 2, 2), "k32": (32, 2, 2), "k33": (33, 2, 2), "k64": (64, 2, 2), "c1": (5, 1, 1)}[name]
    return synth.general(seed=5, m=77, n=45, fu=fu, fv=fv, k=k)


def ref_terms(g, o, ds, freq=False):
    return R.terms(g.get, ds, o.f, o.fu, o.k, o.omega, o.r, o.lam, o.self_side, freq)


def relerr(x, y):
    return abs(x - y) / max(1e-300, abs(y))


def term_errors(ob, ref):
    return {t: relerr(ob[t], ref[t]) for t in TERMS + ("value",)}


# ------------------------------------------------------ 1. oracle parity, fp64
@pytest.mark.parametrize("self_side", [True, False])
@pytest.mark.parametrize("name", ["k5", "k32", "k33", "c1", "tiny"])
def test_oracle_parity_fp64(name, self_side):
    ds = shape(name)
    o, g = pair(ds, self_side=self_side, with_test=False)
    ob = g.objective()
    assert (ob["m"], ob["n"], ob["labels"]) == (ds.train.m, ds.item.m, ds.n_positives)
    e0 = relerr(ob["value"], o.func())
    errs = term_errors(ob, ref_terms(g, o, ds))
    print(f"[objective fp64 {name} self_side={self_side}] init: func {e0:.2e} terms {errs}")
    assert e0 <= 1e-12
    assert max(errs.values()) <= 1e-12, errs
    for _ in range(2):
        o.one_epoch()
        g.one_epoch()
    ob = g.objective()
    e2 = relerr(ob["value"], o.func())
    errs = term_errors(ob, ref_terms(g, o, ds))
    print(f"[objective fp64 {name} self_side={self_side}] 2 epochs: func {e2:.2e} terms {errs}")
    assert e2 <= fp64_tol(ds.name, 2)
    assert max(errs.values()) <= 1e-12, errs


# ------------------------------------------------------------- 2. fp32 problems
@pytest.mark.parametrize("name", ["k32", "k64", "k5"])
def test_fp32_terms(name):
    ds = shape(name)
    o, g = pair(ds, precision=ocffm.FP32, with_test=False)
    for _ in range(2):
        g.one_epoch()
    errs = term_errors(g.objective(), ref_terms(g, o, ds))
    print(f"[objective fp32 {name}] 2 epochs: {errs}")
    assert max(errs.values()) <= 1e-3, errs


def test_fp32_long_rows():
    """20 000 user rows in one table: the fp32 accumulators of a row range are
    widened every 1024 rows, so the error does not grow with the row count."""
    ds = synth.general(seed=5, m=20000, n=300, fu=1, fv=1, k=32)
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP32, with_test=False)
    ocffm.srand(1)
    g.init()
    p = ds.params
    ref = R.terms(g.get, ds, 2, 1, 32, p["w"], p["r"], p["l"])
    errs = term_errors(g.objective(), ref)
    print(f"[objective fp32 m=20000] init: {errs}")
    assert max(errs.values()) <= 1e-3, errs


@pytest.mark.parametrize("precision,bound", [(ocffm.FP32, 1e-3), (ocffm.FP64, 1e-12)])
def test_many_tables(precision, bound):
    """39 cross tables at kp 64, config 5's tile layout at a small row count: 20 groups of 2,
    210 group pairs on grid.y, 780 tile pairs, an odd number of row ranges on either side."""
    ds = synth.general(seed=7, m=150, n=70, fu=13, fv=3, k=33)
    g = ocffm.problem_from_dataset(ds, precision=precision, with_test=False)
    ocffm.srand(1)
    g.init()
    p = ds.params
    errs = term_errors(g.objective(), R.terms(g.get, ds, 16, 13, 33, p["w"], p["r"], p["l"]))
    print(f"[objective many tables precision={precision}] init: {errs}")
    assert max(errs.values()) <= bound, errs


# ------------------------------------------------------------------ 3. --freq
def rederive(g, path):
    """ocffm_problem_set recomputes P / Q only; the biases and the stored
    residual the objective reads are re-derived from W / H by load_binary."""
    g.save_binary(path)
    g.load_binary(path)


@pytest.mark.parametrize("freq", [True, False])
def test_freq_and_gradient_consistency(freq, tmp_path):
    ds = synth.general(seed=5, m=60, n=40, fu=2, fv=2, k=5, nnz_user=2, mean_pos=3.0, vals="real")
    o, g = pair(ds, freq=freq, with_test=False)
    ob = g.objective()
    reg = R.reg_term(g.get, ds, o.f, o.fu, o.k, o.lam, True, freq)
    assert relerr(ob["reg"], reg) <= 1e-12
    if freq:  # the weights are not all one on this set
        assert relerr(reg, R.reg_term(g.get, ds, o.f, o.fu, o.k, o.lam, True, False)) > 1e-3
    path = str(tmp_path / "state.bin")
    rng = np.random.default_rng(3)
    worst = 0.0
    for f1 in range(o.f):
        for f2 in range(f1, o.f):
            b12 = O.block_index(f1, f2, o.f)
            for half, what in enumerate("WH"):
                G = g.grad(f1, f2, half)
                base = g.get(what, b12)
                v = rng.standard_normal(base.size)
                vals = []
                for s in (1.0, -1.0):
                    g.set(what, b12, base + s * 1e-6 * v)
                    rederive(g, path)
                    vals.append(g.objective()["value"])
                g.set(what, b12, base)
                rederive(g, path)
                fd, gv = (vals[0] - vals[1]) / 2e-6, float(G @ v)
                worst = max(worst, abs(fd - gv) / max(1.0, abs(gv)))
                assert abs(fd - gv) <= 1e-5 * max(1.0, abs(gv)), (f1, f2, half, fd, gv)
    print(f"[objective freq={freq}] worst finite-difference mismatch {worst:.2e}")


# --------------------------------------------------------------- 4. read-only
def test_objective_changes_no_state():
    ds = shape("k5")
    gs = []
    for watch in (False, True):
        g = ocffm.problem_from_dataset(ds, precision=ocffm.FP32, with_test=False)
        ocffm.srand(1)
        g.init()
        if watch:
            g.objective()
        for _ in range(2):
            g.one_epoch()
            if watch:
                g.objective()
        gs.append(g)
    o = O.Oracle(ds, with_test=False)
    for b12 in state_names(o):
        for what in "WHPQ":
            np.testing.assert_array_equal(gs[0].get(what, b12), gs[1].get(what, b12))
    for what in "abuvst":
        np.testing.assert_array_equal(gs[0].get(what), gs[1].get(what))
    np.testing.assert_array_equal(gs[0].cg_log(), gs[1].cg_log())


# ---------------------------------------------------- 5. knobs and determinism
def _objective_at(ds, precision, env, monkeypatch):
    for key in ("OCFFM_OBJ_BLOCKS", "OCFFM_OBJ_GROUP", "OCFFM_NO_MFMA"):
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    g = ocffm.problem_from_dataset(ds, precision=precision, with_test=False)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    a, b = g.objective(), g.objective()
    assert a == b  # equal bits from call to call
    return a


@pytest.mark.parametrize("precision,bound", [(ocffm.FP64, 1e-12), (ocffm.FP32, 1e-6)])
def test_knobs_reassociate_only(precision, bound, monkeypatch):
    ds = shape("k32")
    base = _objective_at(ds, precision, {}, monkeypatch)
    worst = 0.0
    envs = [{"OCFFM_OBJ_BLOCKS": b, "OCFFM_OBJ_GROUP": gr} for b in "13" for gr in "13"] + [{"OCFFM_NO_MFMA": "1"}]
    for env in envs:
        ob = _objective_at(ds, precision, env, monkeypatch)
        e = max(relerr(ob[t], base[t]) for t in TERMS + ("value",))
        worst = max(worst, e)
        assert e <= bound, (env, e)
    print(f"[objective knobs precision={precision}] worst relative difference from the default {worst:.2e}")


# ----------------------------------------------------------------- 6. sharding
WORLD = 2


def _dist_dataset(name):
    if name == "owned":  # a listener-id field: its features are owned by one rank's rows (sync_owned)
        return synth.kkbox(seed=5, m=300, n=400, mean=12.0, name="kkbox_dist")
    return synth.tiny(seed=8)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gpu_worker(rank, port, out_dir, world, name):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import ocffm

    def allreduce(arr):
        t = torch.from_numpy(arr)
        dist.all_reduce(t)

    g = ocffm.problem_from_dataset(_dist_dataset(name), precision=ocffm.FP64, rank=rank, nranks=world,
                                   allreduce=allreduce)
    ocffm.srand(1)
    g.init()
    v0 = g.objective()
    g.one_epoch()
    v1 = g.objective()
    np.save(os.path.join(out_dir, f"r{rank}.npy"), np.array([v0["value"], v1["value"], v0["m"], v0["labels"]]))
    g.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("name", ["tiny", "owned"])
def test_two_ranks_match_one_rank(name):
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_gpu_worker, args=(_free_port(), d, WORLD, name), nprocs=WORLD, join=True)
        got = [np.load(os.path.join(d, f"r{r}.npy")) for r in range(WORLD)]
    ds = _dist_dataset(name)
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP64)
    ocffm.srand(1)
    g.init()
    v0 = g.objective()
    g.one_epoch()
    v1 = g.objective()
    for r in range(WORLD):
        e = (relerr(got[r][0], v0["value"]), relerr(got[r][1], v1["value"]))
        print(f"[objective sharded {name}] rank {r}: init {e[0]:.2e}, one epoch {e[1]:.2e}")
        assert (int(got[r][2]), int(got[r][3])) == (ds.train.m, ds.n_positives)
        assert e[0] <= 1e-12 and e[1] <= 1e-12, (r, e)


# --------------------------------------------------------- 7. errors and stats
def test_errors_and_stats(tiny):
    g = ocffm.problem_from_dataset(tiny, precision=ocffm.FP32)
    with pytest.raises(ocffm.OcffmError) as e:
        g.objective()
    assert e.value.code == ocffm.E_STATE
    assert ocffm.lib().ocffm_problem_objective(g.h, None) == ocffm.E_ARG
    ocffm.srand(1)
    g.init()
    g.set_profiling(True)
    g.objective()
    st = g.kernel_stats()["objective"]
    assert st["launches"] > 0 and st["alg_bytes"] > 0 and st["alg_flops"] > 0
    assert g.counter("obj_us") > 0


# ------------------------------------------------------- 8. solve_ex and the CLI
TOL = 0.006


def oracle_sequence(tiny, epochs):
    o = O.Oracle(tiny)
    O.lib().orc_srand(1)
    o.init()
    seq = [o.func()]
    for _ in range(epochs):
        o.one_epoch()
        seq.append(o.func())
    return seq


@pytest.fixture(scope="module")
def tiny_sequence(tiny):
    """The oracle's objective at init and after each of 5 epochs, and the epoch the tolerance stops at."""
    seq = oracle_sequence(tiny, 5)
    dec = [(seq[t] - seq[t + 1]) / abs(seq[t]) for t in range(5)]
    stop = next(t + 1 for t in range(5) if dec[t] <= TOL)
    # the tolerance sits a factor 1.3 clear of the decreases on either side
    assert stop == 4 and dec[2] > 1.3 * TOL and dec[3] < TOL / 1.3, dec
    return seq, stop


def objective_lines(stdout):
    out = []
    for ln in stdout.splitlines():
        if ln.startswith("objective"):
            kv = dict(tok.split("=") for tok in ln.split()[1:])
            out.append((kv["iter"], float(kv["value"]), kv.get("decrease")))
    return out


def test_solve_tol_stops(tiny, tiny_sequence):
    seq, stop = tiny_sequence
    g = ocffm.problem_from_dataset(tiny, precision=ocffm.FP64, t=20)
    ocffm.srand(1)
    g.init()
    rep = g.solve(tol=TOL)
    assert rep["epochs"] == stop == 4 and rep["converged"] is True
    assert relerr(rep["objective0"], seq[0]) <= 1e-9 and relerr(rep["objective"], seq[4]) <= 1e-9
    assert g.cg_log().size == 4 * 2 * 6


def _train(args, tiny, tmp_path):
    paths = tiny.write(str(tmp_path))
    r = subprocess.run([TRAIN] + args + [paths["item"], paths["train"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout, paths


def test_cli_tol(tiny, tiny_sequence, tmp_path):
    seq, stop = tiny_sequence
    paths = tiny.write(str(tmp_path))
    out, _ = _train(["--tol", str(TOL), "-t", "20", "-p", paths["test"]], tiny, tmp_path)
    lines = objective_lines(out)
    assert [ln[0] for ln in lines] == ["init", "1", "2", "3", "4"]
    assert lines[0][2] is None and all(ln[2] is not None for ln in lines[1:])
    for ln, want in zip(lines, seq):
        assert relerr(ln[1], want) <= 1e-9, (ln, want)
    rows = out.splitlines()
    assert rows[0].startswith("iter") and rows[1].startswith("objective iter=init")
    # the early stop's epoch is validated: its table row ends the output, after the last objective line
    assert rows[-2].startswith("objective iter=4") and rows[-1].split()[0] == "4" and len(rows[-1].split()) > 10


def test_cli_objective_flag(tiny, tmp_path):
    out, _ = _train(["--objective", "-t", "3"], tiny, tmp_path)
    assert [ln[0] for ln in objective_lines(out)] == ["init", "1", "2", "3"]
    out, _ = _train(["--objective", "2", "-t", "5"], tiny, tmp_path)
    assert [ln[0] for ln in objective_lines(out)] == ["init", "2", "4"]
    out, _ = _train(["-t", "3"], tiny, tmp_path)
    assert not any(ln.startswith("objective") for ln in out.splitlines())


def test_solve_ex_zero_options_is_solve(tiny, capfd):
    outs = []
    for ex in (False, True):
        g = ocffm.problem_from_dataset(tiny, precision=ocffm.FP64, t=10)
        ocffm.srand(1)
        g.init()
        capfd.readouterr()
        if ex:
            zero = ocffm._SolveOpts(0, 0.0, 0)
            rep = ocffm._SolveReport()
            assert ocffm.lib().ocffm_problem_solve_ex(g.h, zero, rep) == ocffm.OK
            assert (rep.epochs, rep.converged) == (10, 0)
        else:
            assert g.solve() == dict(epochs=10, converged=False, objective0=None, objective=None)
        outs.append(capfd.readouterr().out)
        g.close()
    assert outs[0] == outs[1] and outs[0].startswith("iter") and len(outs[0].splitlines()) == 2
