"""CPU oracle of DBA on a FlatGraph -- TEST INFRASTRUCTURE ONLY.  It restates the reference's
`DbaComputation` (pydcop/algorithms/dba.py:272-597, Yokoo & Hirayama's Distributed Breakout) expression
by expression and is pinned against the reference's own computations by
tests/test_dba_oracle_vs_reference.py.  pydcop_amd/csrc/dba.h follows it value for value.

Both phases park early messages (:358-364, :498-502) and wait for every neighbour (:373, :521), so a
round is bulk-synchronous.  Round r = 1, 2, ...:

State and start
   - neighbours = the other variables of the variable's constraints (:317-318).  A variable without
     any (no constraint, or unary ones only) draws its start value, sends nothing, waits for
     `len(values) == len(neighbors)` in a handler that never runs: it never plays (:341-349, :373).
   - start (:343): `random.choice(domain)`, held cost `current_cost` = None.  The variable's
     initial value is NOT looked at.
   - one integer weight per (variable, constraint) SLOT, from 1 (:311).
1. ok (`_handle_ok_message` :366-391, `improve` :398-420)
   - eval(x) (`compute_eval_value`, :452-482): from 0, over the variable's constraints in order, +=
     the slot's weight where the entry at x, the others at their current values, is `>= INFINITY`.
   - `__cost__ = eval(current value)` (:385).  `__cost__` is the attribute `current_cost` reads (two
     trailing underscores: no name mangling), so the held cost is this eval from round 1 on.
   - `_compute_best_improvement` (:428-445): `best_eval` STARTS AT `INFINITY`; domain order, `<`
     restarts the list, `==` joins it -- a value whose eval is above infinity is never a best value,
     one whose eval EQUALS infinity joins the list.
   - `_consistent = (__cost__ == 0)`; if not, `_termination_counter = 0` (:402-406).
   - `_my_improve = __cost__ - best_eval`; `> 0`: `_can_move`, `_new_value = random.choice(bests)`
     -- with an empty list (every eval above infinity) the reference raises IndexError, and so does
     this oracle; otherwise `_quasi_local_minimum` (:408-415).  `_new_value` keeps its old value
     (None at first) in a round without improvement.
   - the violated slots at the current value are kept (:417-418).
   - sent: (improve, current_eval, termination_counter) (:422-426).
2. improve (`_handle_improve_message`, :504-535), per neighbour, idempotent and commutative:
   - counter = min(counter, theirs) (:509-510)
   - theirs > mine: can_move = False and qlm = False; equal and `self.name > their name`:
     can_move = False (:512-516)
   - their eval > 0: consistent = False (:518-519)
   then `_send_ok` (:537-562):
   - consistent: counter += 1, stop = (counter == max_distance) -- `==` as written
   - unless stopping: qlm -> + 1 on the weight of every slot violated at the ok phase's values;
     can_move -> `value_selection(_new_value, __cost__ - _my_improve)`.
Stop
   - only `min`: the constructor raises ValueError for `max` (:295-298).
   - the reference floods `dba_end` (:544-549, :577-583); which rounds far-away variables still
     complete depends on message timing.  The reading here, the engine's and the reference driver's
     (tests/dba_reference.py): THE RUN ENDS WITH THE FIRST ROUND IN WHICH ANY VARIABLE'S STOP
     CONDITION HOLDS.  Every other variable has done that round's `_send_ok`; nothing after it runs.
     With `max_distance` below the graph's diameter this can leave violated constraints elsewhere:
     the reference's behaviour.

The two draws of the unseeded `random` are `dsa_uniform(seed, v, cycle, draw)` (oracle/ref_harness.py),
seq[int(u * len(seq))] over domain order:

  draw 8  start value                       cycle 0
  draw 9  one of the best values            the computation's cycle_count = r - 1 (`new_cycle` runs in `_send_ok`)
"""
import numpy as np

from gdba_oracle import uniform_vec
from pydcop_amd.graph import FlatGraph, Params
from pydcop_amd.mgm import name_ranks

D_START, D_BEST = 8, 9


class OracleDba:
    def __init__(self, graph: FlatGraph, params: Params = None, infinity=10000, max_distance=50, seed=0):
        g = graph
        self.graph = g
        self.params = params or Params()
        if self.params.mode != "min":
            raise ValueError("DBA is a constraint **satisfaction** algorithm and only support minimization objective")
        if not np.isfinite(infinity):
            raise ValueError("dba: infinity must be finite")
        self.infinity, self.max_distance, self.seed = infinity, int(max_distance), int(seed)
        nV = g.n_vars
        self.dom = [int(d) for d in g.dom_size]
        self.vrow = [int(x) for x in g.var_rowptr]
        self.rank = name_ranks(g.var_names) if g.var_names else np.arange(nV)
        self.violated = np.asarray(g.tables, dtype=np.float64) >= float(infinity)     # NaN: False, +inf: True
        efac = np.repeat(np.arange(g.n_factors), np.diff(g.factor_rowptr))
        self.nS = len(g.var_edges)
        self.slots = []              # per slot: (base, stride of the owner, [(other variable, stride)])
        self.neigh = []
        for v in range(nV):
            nb = set()
            for s in range(self.vrow[v], self.vrow[v + 1]):
                f = int(efac[g.var_edges[s]])
                stride, sv, others = 1, 0, []
                for e in range(g.factor_rowptr[f + 1] - 1, g.factor_rowptr[f] - 1, -1):
                    u = int(g.edge_var[e])
                    if u == v:
                        sv += stride
                    else:
                        others.append((u, stride))
                        nb.add(u)
                    stride *= self.dom[u]
                self.slots.append((int(g.table_off[f]), sv, others))
            self.neigh.append(sorted(nb))
        self.has_nb = np.array([len(n) > 0 for n in self.neigh], dtype=bool)
        deg = [self.vrow[v + 1] - self.vrow[v] for v in range(nV) if self.has_nb[v]]
        # weights and evals are int32 in the engine: (largest slot count) x (1 + rounds) stays below 2^31
        self.max_rounds = (2 ** 31 - 2) // max(deg) - 1 if deg and max(deg) else 2 ** 31 - 1
        # one bit per entry of every playing variable's private copy, in words of 32 values
        self.mask_bytes = 4 * sum(((self.dom[v] + 31) // 32) * int(np.prod([self.dom[u] for u, _ in self.slots[s][2]] or [1]))
                                  for v in range(nV) if self.has_nb[v] for s in range(self.vrow[v], self.vrow[v + 1]))
        self.reset()

    def reset(self):
        nV = self.graph.n_vars
        u0 = uniform_vec(self.seed, np.arange(nV), 0, D_START)
        self.cur = np.array([int(u0[v] * self.dom[v]) for v in range(nV)], dtype=np.int64)
        self.w = np.ones(self.nS, dtype=np.int64)
        self.cost = np.zeros(nV, dtype=np.int64)
        self.has_cost = np.zeros(nV, dtype=np.uint8)
        self.eval = np.zeros(nV, dtype=np.int64)
        self.improve = np.zeros(nV, dtype=np.int64)
        self.newv = np.full(nV, -1, dtype=np.int64)
        self.counter = np.zeros(nV, dtype=np.int64)
        self.consistent = np.zeros(nV, dtype=np.uint8)
        self.rounds = 0
        self.stop_round = 0
        self.moves = 0
        self.increases = 0

    def _evals(self, v, cur):
        """eval(x) of every value and the violated flag of every slot at the current value"""
        D = self.dom[v]
        acc = [0] * D
        viol = []
        for s in range(self.vrow[v], self.vrow[v + 1]):
            base, sv, others = self.slots[s]
            off = base + sum(int(cur[u]) * st for u, st in others)
            for x in range(D):
                if self.violated[off + x * sv]:
                    acc[x] += int(self.w[s])
            viol.append(bool(self.violated[off + int(cur[v]) * sv]))
        return acc, viol

    def _round(self):
        r = self.rounds + 1
        act = [v for v in range(self.graph.n_vars) if self.has_nb[v]]
        cur = self.cur.copy()                    # the values of the ok phase
        draws = uniform_vec(self.seed, np.arange(self.graph.n_vars), r - 1, D_BEST)
        sent, viols, can_move, qlm = {}, {}, {}, {}
        # 1. ok
        for v in act:
            acc, viols[v] = self._evals(v, cur)
            cost = acc[int(cur[v])]
            bests, best = [], self.infinity
            for x, e in enumerate(acc):
                if e < best:
                    best, bests = e, [x]
                elif e == best:
                    bests.append(x)
            consistent = cost == 0
            if not consistent:
                self.counter[v] = 0
            improve = cost - best
            if improve > 0:
                if not bests:
                    raise IndexError("dba: improve > 0 with no best value: every eval is above infinity")
                can_move[v], qlm[v] = True, False
                self.newv[v] = bests[int(draws[v] * len(bests))]
            else:
                can_move[v], qlm[v] = False, True
            self.cost[v], self.has_cost[v] = cost, 1
            self.eval[v], self.improve[v] = cost, int(improve)
            self.consistent[v] = consistent
            sent[v] = (int(improve), cost, int(self.counter[v]))
        # 2. improve, then _send_ok
        stop = False
        for v in act:
            mine = sent[v][0]
            for u in self.neigh[v]:
                imp, ev, cnt = sent[u]
                self.counter[v] = min(self.counter[v], cnt)
                if imp > mine:
                    can_move[v] = qlm[v] = False
                elif imp == mine and self.rank[v] > self.rank[u]:
                    can_move[v] = False
                if ev > 0:
                    self.consistent[v] = 0
            if self.consistent[v]:
                self.counter[v] += 1
                if self.counter[v] == self.max_distance:
                    stop = True
                    continue
            if qlm[v]:
                for k, bad in enumerate(viols[v]):
                    if bad:
                        self.w[self.vrow[v] + k] += 1
                        self.increases += 1
            if can_move[v]:
                self.moves += int(self.newv[v] != self.cur[v])
                self.cur[v] = self.newv[v]
                self.cost[v] = self.eval[v] - self.improve[v]
        self.rounds = r
        if stop:
            self.stop_round = r

    def run(self, n):
        if self.stop_round:
            return
        if self.rounds + int(n) > self.max_rounds:
            raise ValueError("dba: round count past the range of the int32 weights")
        for _ in range(int(n)):
            self._round()
            if self.stop_round:
                break

    @property
    def cycle_count(self):
        return self.rounds

    @property
    def finished(self):
        return self.stop_round != 0

    def state(self):
        return {"idx": self.cur.astype(np.int32), "cost": self.cost.astype(np.int32), "has_cost": self.has_cost.copy(),
                "eval": self.eval.astype(np.int32), "improve": self.improve.astype(np.int32),
                "new": self.newv.astype(np.int32), "counter": self.counter.astype(np.int32),
                "consistent": self.consistent.copy()}

    def weights(self):
        return self.w.astype(np.int32)

    def assignment(self):
        s = self.state()
        return s["idx"], s["cost"].astype(np.float64)

    def violations(self):
        """the number of constraints whose entry under the current assignment is >= infinity"""
        g = self.graph
        n = 0
        for f in range(g.n_factors):
            lin = 0
            for e in range(g.factor_rowptr[f], g.factor_rowptr[f + 1]):
                lin = lin * self.dom[int(g.edge_var[e])] + int(self.cur[int(g.edge_var[e])])
            n += bool(self.violated[int(g.table_off[f]) + lin])
        return n

    def eval_cost(self, idx=None, infinity=float("inf")):
        from gdba_oracle import OracleGdba
        return OracleGdba.eval_cost(self, idx, infinity)

    def close(self):
        pass
