"""`best_every` of the maxsum_gpu plug-in behind the pyDCOP stand-in (tests/standin, driven as tests/plugin_standin_cases.py
drives it) on the emulated engine, in a child process so that the stand-in never shadows the real pyDCOP of the other
tests: the parameter set, the values the proxies report last (the record's), the refusal with devices > 1."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r"""
import os, sys
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
from emu.run_emulated import enable
enable()
import numpy as np
import pytest
import plugin_standin_cases as T
mod = T.load_plugin()
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumEngine
from pydcop_amd.graph import Params

# the reference's five parameters (pydcop/algorithms/maxsum.py:212-220) plus the project's own
mine = {p.name: (p.type, p.values, p.default_value) for p in mod.algo_params}
reference = {"damping": ("float", None, 0.5), "damping_nodes": ("str", ["vars", "factors", "both", "none"], "both"),
             "stability": ("float", None, 0.1), "noise": ("float", None, 0.01),
             "start_messages": ("str", ["leafs", "leafs_vars", "all"], "leafs")}
assert all(mine[k] == v for k, v in reference.items())
assert set(mine) - set(reference) == {"stop_cycle", "precision", "seed", "chunk", "devices", "best_every"}
assert mine["best_every"] == ("int", None, 0)

# the integer colouring whose best state (cycle 30) is not its last: node names keep the generator's order
g = G.random_coloring(60, seed=31, unary_noise=0)
vs = [T.Var("x%%03d" %% i, [0, 1, 2]) for i in range(g.n_vars)]
cons = []
for f in range(g.n_factors):
    a, b = (int(v) for v in g.edge_var[g.factor_rowptr[f]:g.factor_rowptr[f + 1]])
    cons.append(T.Table("c%%03d" %% f, [vs[a], vs[b]], g.tables[g.table_off[f]:g.table_off[f + 1]].reshape(3, 3)))
values, cycles, graph, _ = T._solve_through_plugin(mod, vs, cons, stop_cycle=40, noise=0, best_every=1)
assert cycles == {40}
with MaxSumEngine(graph, Params()) as eng:
    eng.track_best(1, float("inf"))
    eng.run(40)
    best, (final, belief) = eng.best(), eng.assignment()
assert best["cycle"] < 40 and not np.array_equal(best["idx"], final)       # the record is not the last state
for i, name in enumerate(graph.var_names):
    assert values[name][0] == graph.domains[i][int(best["idx"][i])]         # the record's value ...
    assert values[name][1] == belief[i]                                     # ... beside the current belief, as ever
plain, _, _, _ = T._solve_through_plugin(mod, vs, cons, stop_cycle=40, noise=0)
assert [plain[n][0] for n in graph.var_names] == [graph.domains[i][int(final[i])] for i in range(graph.n_vars)]

with pytest.raises(ValueError, match="best_every"):
    T._solve_through_plugin(mod, vs[:2], cons[:0], stop_cycle=2, noise=0, best_every=1, devices=2)
print("ANYTIME-PLUGIN-OK")
"""


def test_maxsum_gpu_best_every_through_the_standin_on_the_emulated_engine():
    r = subprocess.run([sys.executable, "-c", CODE % {"root": ROOT}], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ANYTIME-PLUGIN-OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
