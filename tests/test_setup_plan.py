"""The launch class of every shape of the set-up kernel tests, pinned on the CPU: rows per lane
(choose_vec), panels, residual_rss's workgroups (rss_groups_of), its ticket form and the panels a
wave slot walks, rotate's column groups -- the arithmetic of bmc_plan.h that the library launches
with, run by tests/launch_plan_check.cpp's `setup` sub-command.  tests/test_setup_classes_gpu.py
runs these shapes; if a shape stops reaching the class named beside it in tests/setup_cases.py,
the shape is what has to change."""
import os
import re
import subprocess

import pytest

import setup_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def classes(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("planner") / "launch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe,
                    os.path.join(HERE, "launch_plan_check.cpp")], check=True)
    shapes = sorted({(n, k, int(dt == "f32")) for dt, n, k in list(sc.RSS_CASES) + list(sc.PANELIZE_CASES)} |
                    {(n, k, 0) for n, _, k, _ in sc.ORTHO_CASES})
    args = [str(v) for s in shapes for v in s]
    out = subprocess.run([exe, "setup"] + args, check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        m = re.fullmatch(r"setup n=(\d+) k=(\d+) f32=(\d): vec=(\d+) np=(\d+) rows_per_panel=(\d+) "
                         r"last_rows=(\d+) \| rss G=(\d+) ticket=(flat|two-level) trips=(\d+) \| "
                         r"rotate ncg=(\d+) last_wave_cols=(\d+)", line)
        assert m, line
        v = m.groups()
        got[(int(v[0]), int(v[1]), int(v[2]))] = dict(
            vec=int(v[3]), np=int(v[4]), rows_per_panel=int(v[5]), last_rows=int(v[6]), G=int(v[7]),
            ticket=v[8], trips=int(v[9]), ncg=int(v[10]), last_wave_cols=int(v[11]))
    assert sorted(got) == shapes
    return got


@pytest.mark.parametrize("key", list(sc.RSS_CASES), ids=sc.case_id)
def test_rss_shape_reaches_its_class(classes, key):
    dt, n, k = key
    got = classes[(n, k, int(dt == "f32"))]
    assert {f: got[f] for f in sc.RSS_CASES[key]} == sc.RSS_CASES[key]
    assert got["rows_per_panel"] == 64 * got["vec"]


def test_rss_cases_cover_every_type_and_width():
    """All five (storage type, rows per lane) pairs of residual_rss_kernel, both ticket forms, the
    smallest two-level grid, a ragged last panel and a second trip of the panel loop at one and at
    two rows per lane."""
    have = {(dt, c["vec"]) for (dt, _, _), c in sc.RSS_CASES.items()}
    assert have == {("f64", 1), ("f64", 2), ("f32", 1), ("f32", 2), ("f32", 4)}
    assert {c["ticket"] for c in sc.RSS_CASES.values()} == {"flat", "two-level"}
    assert 257 in {c["G"] for c in sc.RSS_CASES.values()}
    assert {c["vec"] for c in sc.RSS_CASES.values() if c["trips"] == 2} == {1, 2}
    assert all(c["trips"] in (1, 2) for c in sc.RSS_CASES.values())
    assert any(1 < c["last_rows"] < 64 * c["vec"] for c in sc.RSS_CASES.values())
    assert sc.RSS_BATCHES == (1, 2, 3, 4, 5, 8)


@pytest.mark.parametrize("key", list(sc.PANELIZE_CASES), ids=sc.case_id)
def test_panelize_shape_reaches_its_class(classes, key):
    dt, n, k = key
    got = classes[(n, k, int(dt == "f32"))]
    assert {f: got[f] for f in sc.PANELIZE_CASES[key]} == sc.PANELIZE_CASES[key]
    assert got["last_rows"] < got["rows_per_panel"]        # a ragged last panel


@pytest.mark.parametrize("key", list(sc.ORTHO_CASES), ids=sc.case_id)
def test_orthogonalize_shape_reaches_its_class(classes, key):
    n, km, k, pad = key
    got = classes[(n, k, 0)]       # the panels follow the FINAL (n x k) problem (bmc_orthogonalize)
    assert {f: got[f] for f in sc.ORTHO_CASES[key]} == sc.ORTHO_CASES[key]
    assert got["last_rows"] < got["rows_per_panel"] and k <= km - 1


def test_orthogonalize_cases_cover_the_rotate_edges():
    c = sc.ORTHO_CASES
    assert {v["vec"] for v in c.values()} == {1, 2}                      # centre_kernel<1>, <2>
    assert {v["ncg"] for v in c.values()} == {1, 2}
    assert any(v["ncg"] == 2 and k == 33 for (_, _, k, _), v in c.items())   # one column in group 2
    assert any(v["np"] < 8 for v in c.values()) and any(v["np"] > 8 and v["np"] % 8 for v in c.values())
    assert {v["last_wave_cols"] for v in c.values()} >= {1, 7, 8}
    assert any(pad > 0 for (_, _, _, pad) in c)                          # ldf > n_models
