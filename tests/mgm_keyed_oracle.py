"""CPU oracle of MGM with keyed draws on a FlatGraph -- TEST INFRASTRUCTURE ONLY.  It restates the reference's
`MgmComputation` (pydcop/algorithms/mgm.py) the way oracle/mgm_oracle.c does, expression by expression, in f64 or f32
arithmetic (`Params.dtype`), with the reference's two draws from the unseeded `random` either fixed as that oracle
fixes them (`draws="fixed"`: tests/test_mgm_keyed_oracle.py holds the two oracles against each other) or keyed
(`draws="keyed"`), and is pinned against the reference's own computations by
tests/test_mgm_keyed_oracle_vs_reference.py.  pydcop_amd/csrc/mgm.hip follows it bit for bit.

A round is bulk-synchronous (both phases wait for all neighbours and park early messages).  Round k, from 1, is the
computation's `cycle_count` k: the counter starts at 1 and `new_cycle()` runs after the decision (mgm.py:407).

1. values in (`_handle_value_message`, :335-391)
   - first round: cost = reduce(add, [c(current value) for c in constraints]) -- no initial 0 -- plus
     `cost_for_val` of every distinct variable of the constraints (the variable itself included) at its value;
   - `find_arg_optimal` over the domain: strictly better starts a new list, equal joins it; val_cost = the optimum
     plus the same variable costs, the variable's own at its CURRENT value; gain = cost - val_cost;
   - gain > 0 (min) / < 0 (max): new value = random.choice(list), else the current value.
2. gains in (`_handle_gain_message`, :499-588): the largest gain of the neighbourhood moves -- max() also in max
   mode --, ties by name; a variable that moves holds cost - gain.

The variable costs are summed in ascending variable index (the reference iterates a set, see oracle/mgm_oracle.c).
A variable without neighbours takes `optimal_cost_value` at start and never plays.

The draws are `dsa_uniform(seed, v, cycle, draw)` (oracle/ref_harness.py), v the variable's index in the graph,
seq[int(u * len(seq))]:

  draw 10  start value of a variable with neighbours and no initial value      cycle 0
  draw 11  one of the best values, when the gain improves                        cycle k

`late_picks` counts the draws of id 11 that picked an index > 0: what `draws="fixed"` would have decided otherwise.
"""
import numpy as np

from oracle.ref_harness import dsa_uniform
from pydcop_amd.graph import FlatGraph, Params
from pydcop_amd.mgm import name_ranks

D_START, D_BEST = 10, 11


class OracleMgmKeyed:
    def __init__(self, graph: FlatGraph, params: Params = None, draws="fixed", seed=0):
        assert draws in ("fixed", "keyed")
        g = graph
        self.graph = g
        self.params = params or Params()
        self.T = np.float32 if self.params.dtype == "f32" else np.float64
        self.is_max = self.params.mode == "max"
        self.keyed = draws == "keyed"
        self.seed = int(seed) & (2 ** 64 - 1)
        nV = g.n_vars
        self.dom = [int(d) for d in g.dom_size]
        self.tables = g.tables.astype(self.T)
        self.var_cost = g.var_cost.astype(self.T)
        self.cost_off = [int(x) for x in g.cost_off]
        self.rank = name_ranks(g.var_names) if g.var_names else np.arange(nV)
        self.vrank = g.value_rank()
        efac = np.repeat(np.arange(g.n_factors), np.diff(g.factor_rowptr))
        self.slots = []         # per variable: [(base, stride of the variable, [(other variable, stride)])]
        self.conc = []          # per variable: the distinct variables of its constraints, itself included, ascending
        self.has_nb = np.zeros(nV, dtype=bool)
        for v in range(nV):
            mine, seen = [], {v} if g.var_rowptr[v + 1] > g.var_rowptr[v] else set()
            for s in range(int(g.var_rowptr[v]), int(g.var_rowptr[v + 1])):
                f = int(efac[g.var_edges[s]])
                e0, e1 = int(g.factor_rowptr[f]), int(g.factor_rowptr[f + 1])
                if e1 - e0 > 1:
                    self.has_nb[v] = True
                stride, sv, others = 1, 0, []
                for e in range(e1 - 1, e0 - 1, -1):
                    u = int(g.edge_var[e])
                    if u == v:
                        sv += stride
                    else:
                        others.append((u, stride))
                    seen.add(u)
                    stride *= self.dom[u]
                mine.append((int(g.table_off[f]), sv, others))
            self.slots.append(mine)
            self.conc.append(sorted(seen))
        self.reset()

    # ---- state -----------------------------------------------------------------------------------
    def reset(self):
        """on_start (:279-305)"""
        g, T = self.graph, self.T
        nV = g.n_vars
        self.cur = np.zeros(nV, dtype=np.int64)
        self.cost = np.zeros(nV, dtype=T)
        self.has_cost = np.zeros(nV, dtype=np.uint8)
        self.gain = np.zeros(nV, dtype=T)
        self.rounds = 0
        self.late_picks = 0
        for v in range(nV):
            D, o = self.dom[v], self.cost_off[v]
            if self.has_nb[v]:
                if g.init_idx is not None and g.init_idx[v] >= 0:
                    self.cur[v] = g.init_idx[v]
                elif self.keyed:
                    self.cur[v] = int(dsa_uniform(self.seed, v, 0, D_START) * D)
            else:   # optimal_cost_value: min / max over (cost, value) tuples (relations.py:1661-1665)
                c = self.var_cost[o:o + D]
                rk = self.vrank[o:o + D] if self.vrank is not None else np.arange(D)
                keys = [(c[d], rk[d], d) for d in range(D)]
                best = max(keys) if self.is_max else min(keys)
                self.cur[v] = best[2]
                self.cost[v] = best[0]
                self.has_cost[v] = 1
        self.newv = self.cur.copy()

    def _utilities(self, v):
        """reduce(add, [c(x) for c in constraints]) for every x of the domain: utilities order, no initial 0"""
        xs = np.arange(self.dom[v])
        acc = None
        for base, sv, others in self.slots[v]:
            off = base + sum(int(self.cur[u]) * st for u, st in others)
            vals = self.tables[off + xs * sv]
            acc = vals if acc is None else (acc + vals).astype(self.T)
        return acc

    def _add_var_costs(self, v, acc):
        for u in self.conc[v]:      # own: the current value; neighbours: theirs
            acc = self.T(acc + self.var_cost[self.cost_off[u] + int(self.cur[u])])
        return acc

    def _round(self):
        T = self.T
        k = self.rounds + 1
        act = np.flatnonzero(self.has_nb)
        for v in act:                                   # 1. values in
            ut = self._utilities(v)
            if not self.has_cost[v]:
                self.cost[v] = self._add_var_costs(v, ut[self.cur[v]])
                self.has_cost[v] = 1
            best, lst = ut[0], [0]
            for x in range(1, self.dom[v]):
                if (best < ut[x]) if self.is_max else (best > ut[x]):
                    best, lst = ut[x], [x]
                elif ut[x] == best:
                    lst.append(x)
            val_cost = self._add_var_costs(v, best)
            gain = T(self.cost[v] - val_cost)
            self.gain[v] = gain
            if (gain < 0) if self.is_max else (gain > 0):
                j = int(dsa_uniform(self.seed, int(v), k, D_BEST) * len(lst)) if self.keyed else 0
                self.late_picks += j > 0
                self.newv[v] = lst[j]
            else:
                self.newv[v] = self.cur[v]
        cur2, cost2 = self.cur.copy(), self.cost.copy()
        for v in act:                                   # 2. gains in
            nb = [u for u in self.conc[v] if u != v]
            max_n = max(self.gain[u] for u in nb)
            wins = not any(self.gain[u] == max_n and self.rank[u] < self.rank[v] for u in nb)
            if self.gain[v] > max_n or (self.gain[v] == max_n and wins):
                cur2[v] = self.newv[v]
                cost2[v] = T(self.cost[v] - self.gain[v])
        self.cur, self.cost = cur2, cost2
        self.rounds += 1

    def run(self, n):
        for _ in range(int(n)):
            self._round()

    @property
    def cycle_count(self):
        return self.rounds

    def state(self):
        return {"idx": self.cur.astype(np.int32), "cost": self.cost.astype(np.float64),
                "has_cost": self.has_cost.copy(), "gain": self.gain.astype(np.float64),
                "new": self.newv.astype(np.int32)}

    def assignment(self):
        s = self.state()
        return s["idx"], s["cost"]

    def eval_cost(self, idx=None, infinity=float("inf")):
        """DCOP.solution_cost (pydcop/dcop/dcop.py:308-367): constraints, then variable costs, in index order."""
        g = self.graph
        idx = self.cur if idx is None else np.asarray(idx)
        lin = np.zeros(g.n_factors, dtype=np.int64)
        arity = np.diff(g.factor_rowptr)
        for j in range(int(arity.max()) if g.n_factors else 0):
            a = j < arity
            u = g.edge_var[np.where(a, g.factor_rowptr[:-1] + j, 0)]
            lin = np.where(a, lin * g.dom_size[u] + idx[u], lin)
        x = g.tables[g.table_off[:-1] + lin]
        ev = g.eval_var_cost if g.eval_var_cost is not None else g.var_cost
        y = ev[np.asarray(g.cost_off[:-1]) + idx]
        soft, hard = 0.0, 0
        for t in (x, y):
            for e in t:
                if e != infinity:
                    soft += float(e)
                else:
                    hard += 1
        return soft, hard

    def close(self):
        pass
