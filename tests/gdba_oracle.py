"""CPU oracle of GDBA on a FlatGraph -- TEST INFRASTRUCTURE ONLY.  It restates the reference's
`GdbaComputation` (pydcop/algorithms/gdba.py:189-658) expression by expression, in f64 or f32
arithmetic (`Params.dtype`), and is pinned against the reference's own computations by
tests/test_gdba_oracle_vs_reference.py.  pydcop_amd/csrc/gdba.h follows it bit for bit.

Both phases wait for all neighbours and park early messages, so a round is bulk-synchronous.
Round r (the computation's `cycle_count`, from 1):

1. ok (`_handle_ok_message`, :352-387)
   - eval(x) (`compute_eval_value`, :428-461), from 0 over the variable's constraints in
     `node.constraints` order: `+= eff_cost(c, x)`, then `+= vars_cost`, INSIDE the loop.
     eff_cost = table entry + modifier (`modifier: A`) or * modifier (`M`), the modifier looked up
     under the assignment filtered to the constraint's scope (`_eff_cost`, :574-597).
     vars_cost = the sum, from 0, of `cost_for_val` over a set of (variable, value) that GROWS over
     the loop (the variables of the constraints seen so far, the owner at its CURRENT value, not at
     x): earlier constraints' variables are counted again at every later constraint.
   - cost = eval(current value), and the constraints violated AT THE CURRENT VALUE (`_is_violated`,
     :552-572), on the RAW table entry: NZ != 0, NM != min of the flattened table, MX == its max.
   - best (`_compute_best_improvement`, :395-417): strictly better starts a new list, equal joins
     it, domain order.  improve = cost - best; new value = a random one of the best values when
     improve > 0 (min) / < 0 (max), else the current value.
2. improve (`_handle_improve_message`, :493-541)
   - maxi / max_list over the neighbours with `>` and `==` in BOTH modes.
   - improve > 0 (min) / < 0 (max): moves iff sorted(max_list)[0] is its own name; the reported
     cost is then cost + improve, as written.  Nothing else happens in that branch.
   - else, if maxi == 0: every violated constraint is increased (`_increase_cost`, :627-654).

Modifiers (`__constraints_modifiers__`): one table per (variable, constraint), a defaultdict whose
default is 0 (A) or 1 (M), increments of +1: integer counters.  E, R and C write under the
UNFILTERED assignment of all neighbours plus self, the look-ups read under the assignment filtered
to the scope: an increase is only ever read back for a pair whose scope equals {v} + neighbours(v)
(a LIVE slot); for every other pair it is dead, and is not stored here.  E: the entry of the current
assignment; R: that entry for every value of v; C: every assignment of the neighbours with v at its
current value.  T enumerates the constraint's own dimensions: always live, every entry + 1 -- one
counter per slot.

Other quirks kept: a variable without neighbours takes `optimal_cost_value` at start and never
plays (:304-315); there is no stop condition (the caller counts rounds); the held cost is None
until round 1.

Determinism: `vars_cost` iterates a Python set of (Variable, value) whose order follows string
hashes, i.e. it is NOT fixed between processes; the sum is taken here in ascending graph index.
Pinned cases use variable costs whose sums are exact in any order (integers, small dyadic
fractions).  The two draws of the unseeded `random` are `dsa_uniform(seed, v, cycle, draw)`
(oracle/ref_harness.py), seq[int(u * len(seq))] over domain order:

  draw 6  start value of a variable without initial value      cycle 0
  draw 7  one of the best values                                 cycle r
"""
import numpy as np

from pydcop_amd.graph import FlatGraph, Params
from pydcop_amd.mgm import name_ranks

MODIFIERS = ("A", "M")
VIOLATIONS = ("NZ", "NM", "MX")
INCREASE_MODES = ("E", "R", "C", "T")
D_START, D_BEST = 6, 7
MAX_ROUNDS = 65535      # the engine's counters are 16 bits wide

_M = np.uint64
_GOLD = _M(0x9E3779B97F4A7C15)


def _mix64(z):
    z = (z ^ (z >> _M(30))) * _M(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _M(27))) * _M(0x94D049BB133111EB)
    return z ^ (z >> _M(31))


def uniform_vec(seed, variables, cycle, draw):
    """oracle.ref_harness.dsa_uniform over an array of variables (wrapping uint64 arithmetic)."""
    with np.errstate(over="ignore"):
        v = np.asarray(variables).astype(np.uint64)
        z = _M(seed & (2 ** 64 - 1)) + _GOLD * (v + _M(1))
        z = _mix64(z) + _GOLD * _M(cycle + 1)
        z = _mix64(z) + _M(draw)
        return (_mix64(z) >> _M(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


class OracleGdba:
    def __init__(self, graph: FlatGraph, params: Params = None, modifier="A", violation="NZ", increase_mode="E",
                 seed=0):
        g = graph
        assert modifier in MODIFIERS and violation in VIOLATIONS and increase_mode in INCREASE_MODES
        self.graph = g
        self.params = params or Params()
        self.T = np.float32 if self.params.dtype == "f32" else np.float64
        self.is_max = self.params.mode == "max"
        self.modifier, self.violation, self.increase_mode, self.seed = modifier, violation, increase_mode, int(seed)
        self.mod_base = 0 if modifier == "A" else 1
        nV = g.n_vars
        self.dom = g.dom_size.astype(np.int64)
        self.vrow = g.var_rowptr.astype(np.int64)
        self.tables = g.tables.astype(self.T)
        self.var_cost = g.var_cost.astype(self.T)
        self.cost_off = np.asarray(g.cost_off, dtype=np.int64)
        self.has_vc = bool((g.var_cost != 0).any())
        self.rank = name_ranks(g.var_names) if g.var_names else np.arange(nV)
        self.vrank = g.value_rank()
        efac = np.repeat(np.arange(g.n_factors), np.diff(g.factor_rowptr))
        nS = len(g.var_edges)
        self.nS = nS
        self.base = np.zeros(nS, dtype=np.int64)
        self.stride_v = np.zeros(nS, dtype=np.int64)
        self.size = np.zeros(nS, dtype=np.int64)
        self.slot_var = np.repeat(np.arange(nV), np.diff(self.vrow))
        self.slot_pos = np.arange(nS) - self.vrow[self.slot_var]
        live = np.zeros(nS, dtype=bool)
        vref = np.zeros(nS, dtype=self.T)
        fref = np.zeros(g.n_factors, dtype=self.T)    # what a raw entry is compared with: 0, the table's min or max
        if violation != "NZ" and g.n_factors:
            red = np.minimum if violation == "NM" else np.maximum
            fref = red.reduceat(self.tables, g.table_off[:-1].astype(np.int64))
        nbs = []
        self.neigh = []
        self.conc, self.conc_first = [], []
        for v in range(nV):
            first = {v: 0}
            scopes = []
            for s in range(self.vrow[v], self.vrow[v + 1]):
                f = int(efac[g.var_edges[s]])
                self.base[s] = g.table_off[f]
                self.size[s] = g.table_off[f + 1] - g.table_off[f]
                vref[s] = fref[f]
                stride, sv, lst = 1, 0, []
                for e in range(g.factor_rowptr[f + 1] - 1, g.factor_rowptr[f] - 1, -1):
                    u = int(g.edge_var[e])
                    if u == v:
                        sv += stride
                    else:
                        lst.append((u, stride))
                        first.setdefault(u, s - int(self.vrow[v]))
                    stride *= int(self.dom[u])
                self.stride_v[s] = sv
                nbs.append(lst)
                scopes.append({u for u, _ in lst})
            conc = sorted(first)
            self.conc.append(conc)
            self.conc_first.append([first[u] for u in conc])
            self.neigh.append([u for u in conc if u != v])
            for k, sc in enumerate(scopes):             # the scope is {v} + every neighbour of v
                live[self.vrow[v] + k] = len(sc) == len(conc) - 1
        J = max([len(l) for l in nbs] + [1])
        self.nbv = np.full((max(nS, 1), J), -1, dtype=np.int64)
        self.nbs = np.zeros((max(nS, 1), J), dtype=np.int64)
        for s, l in enumerate(nbs):
            for j, (u, st) in enumerate(l):
                self.nbv[s, j], self.nbs[s, j] = u, st
        self.vref = vref
        self.conc_rowptr = np.concatenate([[0], np.cumsum([len(c) for c in self.conc])]).astype(np.int64)
        self.conc_flat = np.array([u for c in self.conc for u in c] + [0], dtype=np.int64)
        self.conc_first_flat = np.array([f for c in self.conc_first for f in c] + [0], dtype=np.int64)
        self.has_nb = np.array([len(n) > 0 for n in self.neigh], dtype=bool)
        NB = max([len(n) for n in self.neigh] + [1])
        self.nb_mat = np.full((nV, NB), -1, dtype=np.int64)
        for v, n in enumerate(self.neigh):
            self.nb_mat[v, :len(n)] = n
        # the modifier pool: one counter per entry of a live slot (E, R, C), one per slot (T)
        self.live = live & self.has_nb[self.slot_var] if nS else live
        self.mod_off = np.full(max(nS, 1), -1, dtype=np.int64)
        stored = self.live if increase_mode != "T" else (self.has_nb[self.slot_var] if nS else live)
        ls = np.flatnonzero(stored)
        per = self.size[ls] if increase_mode != "T" else np.ones(len(ls), dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        self.mod_off[ls] = offs[:-1]
        self.pool_size = int(offs[-1])
        self.reset()

    # ---- state -----------------------------------------------------------------------------------
    def reset(self):
        """on_start (:302-333)"""
        g, T = self.graph, self.T
        nV = g.n_vars
        self.pool = np.zeros(max(self.pool_size, 1), dtype=np.int64)
        self.cur = np.zeros(nV, dtype=np.int64)
        self.cost = np.zeros(nV, dtype=T)
        self.has_cost = np.zeros(nV, dtype=np.uint8)
        self.improve = np.zeros(nV, dtype=T)
        self.rounds = 0
        self.moves = 0
        u0 = uniform_vec(self.seed, np.arange(nV), 0, D_START)
        for v in range(nV):
            if self.has_nb[v]:
                if g.init_idx is not None and g.init_idx[v] >= 0:
                    self.cur[v] = g.init_idx[v]
                else:
                    self.cur[v] = int(u0[v] * self.dom[v])
            else:   # optimal_cost_value: min / max over (cost, value) tuples (relations.py:1661-1665)
                c = self.var_cost[self.cost_off[v]:self.cost_off[v] + self.dom[v]]
                rk = (self.vrank[self.cost_off[v]:self.cost_off[v] + self.dom[v]] if self.vrank is not None
                      else np.arange(self.dom[v]))
                keys = [(c[d], rk[d], d) for d in range(self.dom[v])]
                best = max(keys) if self.is_max else min(keys)
                self.cur[v] = best[2]
                self.cost[v] = best[0]
                self.has_cost[v] = 1
        self.newv = self.cur.copy()

    def _nb_offset(self, s, cur):
        off = np.zeros(len(s), dtype=np.int64)
        for j in range(self.nbv.shape[1]):
            w = self.nbv[s, j]
            off += np.where(w >= 0, cur[np.maximum(w, 0)] * self.nbs[s, j], 0)
        return off

    def _slot_var_costs(self):
        """vars_cost after each slot: the owner and every variable of the constraints so far, ascending index"""
        T = self.T
        vc = np.zeros(max(self.nS, 1), dtype=T)
        if self.nS == 0:
            return vc
        vals = self.var_cost[self.cost_off[:-1] + self.cur]
        v = self.slot_var
        n_conc = self.conc_rowptr[v + 1] - self.conc_rowptr[v]
        acc = vc[:self.nS]
        for c in range(int(n_conc.max())):
            k = np.where(c < n_conc, self.conc_rowptr[v] + c, 0)
            inc = (c < n_conc) & (self.conc_first_flat[k] <= self.slot_pos)
            acc = np.where(inc, (acc + vals[self.conc_flat[k]]).astype(T), acc)
        vc[:self.nS] = acc
        return vc

    def _round(self):
        T = self.T
        r = self.rounds + 1
        if r > MAX_ROUNDS:
            raise ValueError("gdba: round count past the range of the modifier counters")
        act = np.flatnonzero(self.has_nb)
        if len(act) == 0:
            self.rounds += 1
            return
        cur = self.cur
        # 1. ok: eval(x) for every value of every playing variable
        D = self.dom[act]
        qoff = np.concatenate([[0], np.cumsum(D)])
        vq = np.repeat(act, D)
        xq = np.arange(qoff[-1]) - np.repeat(qoff[:-1], D)
        s0 = self.vrow[vq]
        deg = self.vrow[vq + 1] - s0
        vc = self._slot_var_costs() if self.has_vc else None
        acc = np.zeros(len(vq), dtype=T)
        viol = np.zeros(max(self.nS, 1), dtype=bool)
        is_cur = xq == cur[vq]
        for k in range(int(deg.max())):
            a = k < deg
            s = np.where(a, s0 + k, 0)
            idx = xq * self.stride_v[s] + self._nb_offset(s, cur)
            tv = self.tables[np.where(a, self.base[s] + idx, 0)]
            mo = self.mod_off[s]
            if self.increase_mode == "T":
                cnt = self.pool[np.where(a, mo, 0)]
            else:
                cnt = np.where(mo >= 0, self.pool[np.where(a & (mo >= 0), mo + idx, 0)], 0)
            m = (self.mod_base + cnt).astype(T)
            eff = (tv * m if self.modifier == "M" else tv + m).astype(T)
            acc = np.where(a, (acc + eff).astype(T), acc)
            if vc is not None:
                acc = np.where(a, (acc + vc[s]).astype(T), acc)
            bad = (tv == self.vref[s]) if self.violation == "MX" else (tv != self.vref[s])
            sel = a & is_cur
            viol[s[sel]] = bad[sel]
        cost = acc[is_cur]                       # one per playing variable, in `act` order
        # best values: strictly better restarts the list, equal joins it
        n = len(act)
        best = acc[qoff[:-1]].copy()
        n_best = np.ones(n, dtype=np.int64)
        for x in range(1, int(D.max())):
            a = x < D
            e = acc[np.where(a, qoff[:-1] + x, 0)]
            better = a & ((e > best) if self.is_max else (e < best))
            equal = a & (e == best)
            best = np.where(better, e, best)
            n_best = np.where(better, 1, n_best + equal)
        improve = (cost - best).astype(T)
        improving = (improve < 0) if self.is_max else (improve > 0)
        kth = (uniform_vec(self.seed, act, r, D_BEST) * n_best).astype(np.int64)
        newv = cur[act].copy()
        seen = np.zeros(n, dtype=np.int64)
        for x in range(int(D.max())):
            a = x < D
            e = acc[np.where(a, qoff[:-1] + x, 0)]
            hit = a & (e == best)
            take = improving & hit & (seen == kth)
            newv = np.where(take, x, newv)
            seen += hit
        self.cost[act] = cost
        self.has_cost[act] = 1
        self.improve[act] = improve
        self.newv[act] = newv
        # 2. improve: maxi / max_list with > and == in both modes, ties by name
        mine = self.improve[act]
        maxi = mine.copy()
        wins = np.ones(n, dtype=bool)
        for j in range(self.nb_mat.shape[1]):
            u = self.nb_mat[act, j]
            ok = u >= 0
            gu = self.improve[np.maximum(u, 0)]
            gt = ok & (gu > maxi)
            eq = ok & (gu == maxi) & (self.rank[np.maximum(u, 0)] < self.rank[act])
            maxi = np.where(gt, gu, maxi)
            wins &= ~(gt | eq)
        move = improving & wins
        increase = ~improving & (maxi == 0)
        inc_var = np.zeros(self.graph.n_vars, dtype=bool)
        inc_var[act[increase]] = True
        S = np.flatnonzero(viol[:self.nS] & inc_var[self.slot_var])
        S = S[self.mod_off[S] >= 0]
        if self.increase_mode == "T":
            self.pool[self.mod_off[S]] += 1
        else:
            nb = self._nb_offset(S, cur)
            if self.increase_mode == "E":
                self.pool[self.mod_off[S] + cur[self.slot_var[S]] * self.stride_v[S] + nb] += 1
            elif self.increase_mode == "R":
                for s, o in zip(S, nb):
                    v = self.slot_var[s]
                    self.pool[self.mod_off[s] + np.arange(self.dom[v]) * self.stride_v[s] + o] += 1
            else:
                for s in S:
                    v = self.slot_var[s]
                    idx = np.array([cur[v] * self.stride_v[s]], dtype=np.int64)
                    for j in range(self.nbv.shape[1]):
                        w = self.nbv[s, j]
                        if w >= 0:
                            idx = (idx[:, None] + np.arange(self.dom[w])[None, :] * self.nbs[s, j]).ravel()
                    self.pool[self.mod_off[s] + idx] += 1
        mv = act[move]
        self.cur[mv] = self.newv[mv]
        self.cost[mv] = (self.cost[mv] + self.improve[mv]).astype(T)
        self.moves += len(mv)
        self.rounds += 1

    def run(self, n):
        if self.rounds + int(n) > MAX_ROUNDS:
            raise ValueError("gdba: round count past the range of the modifier counters")
        for _ in range(int(n)):
            self._round()

    @property
    def cycle_count(self):
        return self.rounds

    def state(self):
        return {"idx": self.cur.astype(np.int32), "cost": self.cost.astype(np.float64),
                "has_cost": self.has_cost.copy(), "improve": self.improve.astype(np.float64),
                "new": self.newv.astype(np.int32)}

    def assignment(self):
        s = self.state()
        return s["idx"], s["cost"]

    def modifiers(self, slot):
        """The modifier table of slot (variable, its k-th constraint) = var_rowptr[v] + k, in the layout of the
        constraint's table; one entry in mode T; empty where the slot stores none (dead in E, R, C)."""
        mo = self.mod_off[slot]
        if mo < 0:
            return np.zeros(0, dtype=np.int32)
        n = 1 if self.increase_mode == "T" else int(self.size[slot])
        return (self.mod_base + self.pool[mo:mo + n]).astype(np.int32)

    def eval_cost(self, idx=None, infinity=float("inf")):
        """DCOP.solution_cost (pydcop/dcop/dcop.py:308-367): constraints and variable costs."""
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
