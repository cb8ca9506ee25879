"""CPU checks of the simplex chain axis: the launch plan of bmc_plan.h's plan_simplex_launches (g++
builds tests/simplex_plan_check.cpp), the declaration and binding of bmc_simplex_run_chains, and
the argument errors of gibbs_sampler_simplex that are raised before any device is touched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pybmc_amd import _lib, gibbs_sampler_simplex

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pybmc_amd.h")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp_path_factory.mktemp("simplex_plan") / "simplex_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "simplex_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def plan(exe, n, k, km, chains, cu=0, G=0, W=0, res=0, ppw=0, f32=0):
    r = subprocess.run([exe, "plan"] + [str(v) for v in (n, k, f32, km, chains, cu, G, W, res, ppw)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    geo, kernel, launches = r.stdout.strip().split(" | ")
    geo = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in geo.split())
    launches = [tuple(int(x) for x in re.split(r"[+/]", item)) for item in launches.split(";")]
    return geo, kernel, launches   # launches: (c0, chains, nslot, resident workgroups)


def test_plan_sweep(plan_exe):
    """Every chain exactly once and in order, the one-chain geometry and kernel, no launch beyond
    the resident workgroups cu_limit allows -- over shapes x models x chains x cu_limit x tuning."""
    r = subprocess.run([plan_exe, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "sweep" and int(last[1]) > 100000 and int(last[2]) == 0, r.stdout[-2000:]


def test_one_wave_chains_share_one_launch(plan_exe):
    # the reference's size, a model per lane: one wave per chain, 256 chains in one launch
    geo, kernel, launches = plan(plan_exe, 629, 3, 4, 256)
    assert geo["one_wave"] == 1 and geo["waves"] == 1 and kernel == "simplex_wave_kernel<double, 12, 4, false>"
    assert launches == [(0, 256, 256, 256)]
    # four waves per chain
    geo, kernel, launches = plan(plan_exe, 2500, 3, 4, 64)
    assert geo["one_wave"] == 1 and geo["waves"] == 4 and kernel == "simplex_wave_kernel<double, 12, 4, true>"
    assert launches == [(0, 64, 64, 64)]
    # the grid bound
    assert [l[:2] for l in plan(plan_exe, 629, 3, 4, 2049)[2]] == [(0, 2048), (2048, 1)]
    # more than 64 models: no lane per model, the workgroup form (one workgroup per chain and CU)
    geo, kernel, launches = plan(plan_exe, 629, 3, 65, 300)
    assert geo["one_wave"] == 0 and geo["G"] == 1 and kernel.startswith("simplex_loop_kernel<")
    assert [l[:2] for l in launches] == [(0, 256), (256, 44)]


def test_workgroup_chains_fill_the_resident_groups(plan_exe):
    # 32 groups per chain on one XCD each: 8 chains per launch under the XCD labelling
    geo, kernel, launches = plan(plan_exe, 10000, 32, 65, 20)
    assert geo["G"] == 32 and kernel == "simplex_loop_kernel<double, 1, 0, 32, 1, false>"
    assert launches == [(0, 8, 8, 256), (8, 8, 8, 256), (16, 4, 8, 128)]
    # the same kernel for one chain, on the grid bmc_simplex_run has always used (8 slots x 32)
    assert plan(plan_exe, 10000, 32, 65, 1) == (geo | {"max_per_launch": 1}, kernel, [(0, 1, 8, 32)])
    # cu_limit lowers the chains per launch: forced geometries on few CUs
    geo, kernel, launches = plan(plan_exe, 150, 4, 6, 5, cu=6, G=3, W=1, res=1, ppw=1)
    assert geo["G"] == 3 and kernel == "simplex_loop_kernel<double, 1, 0, 8, 1, false>"
    assert launches == [(0, 2, 2, 6), (2, 2, 2, 6), (4, 1, 1, 3)]
    geo, kernel, launches = plan(plan_exe, 150, 4, 6, 5, cu=2, G=1, W=3, res=1, ppw=1)
    assert geo["G"] == 1 and kernel == "simplex_loop_kernel<double, 1, 0, 8, 1, true>"
    assert launches == [(0, 2, 2, 2), (2, 2, 2, 2), (4, 1, 1, 1)]


def test_header_declares_and_python_binds_the_entry_point():
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"int bmc_simplex_run_chains\(([^;]*)\);", text)
    assert m, "include/pybmc_amd.h does not declare bmc_simplex_run_chains"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 21
    assert "n_chains" in params[4] and "seeds" in params[11] and "n_unif" in params[15]
    restype, argtypes = _lib.PROTOTYPES["bmc_simplex_run_chains"]
    assert len(argtypes) == len(params)
    assert hasattr(_lib.Context, "simplex_run_chains")
    assert "bmc_simplex_run" in _lib.PROTOTYPES      # the one-chain entry point stays


def test_seed_arguments_are_checked_before_any_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a context was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "default_context", no_device)
    y = np.array([1.0, 2.0, 3.0])
    X = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    Vt_hat = np.array([[0.5, 0.5], [0.5, -0.5]])
    S_hat = np.array([1.0, 0.5])
    args = (y, X, Vt_hat, S_hat, 10, [1.0, 1.0])
    with pytest.raises(ValueError, match="seed"):
        gibbs_sampler_simplex(*args, seed=1, seeds=[1, 2], n_chains=2)
    with pytest.raises(ValueError, match="seeds"):
        gibbs_sampler_simplex(*args, seeds=[1, 2, 3], n_chains=2)
    with pytest.raises(ValueError, match="seeds"):
        gibbs_sampler_simplex(*args, seeds=[1, 2])          # n_chains = 1
    with pytest.raises(ValueError):
        gibbs_sampler_simplex(*args, n_chains=0)
    # the reference's own checks still come first
    with pytest.raises(ValueError, match="Burn-in"):
        gibbs_sampler_simplex(*args, burn=-1, n_chains=2, seeds=[1, 2])


def test_train_refuses_devices_with_the_simplex_sampler():
    import pandas as pd
    from pybmc_amd import BayesianModelCombination
    df = pd.DataFrame({"model1": [1, 2], "model2": [3, 4], "truth": [5, 6]})
    bmc = BayesianModelCombination(["model1", "model2"], {"property": df}, "truth")
    bmc.U_hat = np.zeros((2, 1))        # as after orthogonalize(): train() only needs the shapes here
    bmc.S_hat = np.ones(1)
    bmc.Vt_hat = np.zeros((1, 2))
    with pytest.raises(ValueError, match="simplex"):
        bmc.train({"iterations": 10, "sampler": "simplex", "burn": 1, "stepsize": 0.01,
                   "b_mean_prior": np.zeros(1), "b_mean_cov": np.eye(1), "nu0_chosen": 1.0,
                   "sigma20_chosen": 0.02, "devices": [0, 1]})


def test_replay_seed_lists_follow_the_rule():
    """The chains of the GPU replay test: the pinned stream seeds are what census_common's rule
    selects, every chain both accepts and rejects and decides with a margin >= MARGIN."""
    import census_common as cc
    import simplex_chain_cases as S
    tt = cc.BURN_SIMPLEX + cc.T_SIMPLEX
    for name, case in S.CASES.items():
        base, chains = S.chains_of(case)
        assert [c["seed"] for c in chains] == case["seeds"], name
        assert len({c["seed"] for c in chains}) == S.N_CHAINS
        for c in chains:
            assert c["margin"] >= cc.MARGIN and tt / 8 < c["acc_all"] < 7 * tt / 8, (name, c["seed"])
