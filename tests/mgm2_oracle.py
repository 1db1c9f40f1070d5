"""CPU oracle of MGM-2 on a FlatGraph -- TEST INFRASTRUCTURE ONLY.  It restates the reference's
`Mgm2Computation` (pydcop/algorithms/mgm2.py:399-1062) expression by expression, in f64 or f32
arithmetic (`Params.dtype`), and is pinned against the reference's own computations by
tests/test_mgm2_oracle_vs_reference.py.  pydcop_amd/csrc/mgm2.h follows it bit for bit.

Every phase waits for all neighbours and parks early messages (`_enter_state`), so a round is
bulk-synchronous.  Round r (the computation's `cycle_count`, from 1):

1. value (`_handle_value_messages`, :742-786)
   - lcost = sum of the variable's constraints, in `node.constraints` order, at the current values,
     from 0 (`assignment_cost`, relations.py:1513-1531, via `_compute_cost`): it becomes the held
     cost (`__cost__`).
   - offerer iff `uniform(0, 1) < threshold`; an offerer picks its partner uniformly among its
     distinct neighbours.
   - an offerer's table (`_compute_offers_to_send`, :521-554): for every (x, y) of D_v x D_p the cost
     over ALL its constraints with itself at x, the partner at y, the others unchanged; kept where it
     strictly improves on lcost (`>` min, `<` max), as lcost - cost.
   - best unilateral move (`_compute_best_value`, :497-519): strictly better starts a new list, equal
     values join it in domain order; pg = lcost - best; pv = a random one of the best values when pg
     is an improvement (`> 0` min, `< 0` max), else the current value.
2. offer (`_handle_offer_messages`, :787-856)
   - an offerer rejects every offer it receives.
   - a non-offerer evaluates each entry of each offer aimed at it (`_find_best_offer`, :556-603):
     global_gain = (lcost - cost_concerned) + partner_gain, cost_concerned summed from 0 over its
     constraints that do NOT contain the offerer, in order; best starts at 0, strictly better (`>`
     min, `<` max) restarts the list of best offers, equal joins it.
   - commits iff gain != 0 and the list is not empty, and gain beats pg (`>` min, `<` max), or
     equals it with favor == coordinated, or with favor == no and `uniform(0, 1) > 0.5`.
   - a committed receiver accepts a random one of the best offers (pv, pg = gain, partner).
3. answer (`_handle_response_message`, :858-890): an offerer whose partner accepted takes the
   accepted value and the global gain and is committed.
4. gain (`_handle_gain_messages`, :892-972)
   - pg == 0: nothing this round.
   - committed: can_move iff no neighbour but the partner, or pg > max(their gains); go(can_move)
     to the partner.
   - otherwise: moves iff pg > max(all neighbours' gains); on equality iff its name is the first of
     sorted(tied neighbours + itself).  A move is value_selection(pv, lcost - pg).
5. go (:974-1001): a committed variable moves iff its partner said go and its own can_move holds.

Quirks kept as they are:
- variable costs are ignored (`assignment_cost` without `consider_variable_cost`); only the final
  `solution_cost` (eval_cost) includes them.
- max mode is half flipped: phases 1-2 flip `<` / `>`, phase 4 compares with `>` and max() in both.
- a committed pair reports the GLOBAL gain as its gain and in its held cost (lcost - pg).
- a variable without neighbours takes a random best value of its own constraints at start (cost =
  that best) and is finished (:460-470).
- `stop_cycle: n` runs n - 1 rounds (`_send_value` calls new_cycle() before the check, :659-672);
  `stop_cycle: 1` runs none.
- initial value: `initial_value` when set, else a random value.

Determinism: every draw of the reference's unseeded `random` is `dsa_uniform(seed, v, cycle, draw)`
(oracle/ref_harness.py, the generator of DSA), `uniform(a, b) = a + (b - a) * u`, and a choice
picks seq[int(u * len(seq))] of a canonically ordered sequence:

  draw 0  start: initial value / best value of a variable without neighbours  cycle 0, domain order
  draw 1  offerer test                                                         cycle r
  draw 2  partner                                     cycle r, distinct neighbours by graph index
  draw 3  one of the best unilateral values                               cycle r, domain order
  draw 4  the `favor: no` coin                                                 cycle r
  draw 5  one of the tied best offers      cycle r, (offerer index, offerer value, own value)
"""
import numpy as np

from oracle.ref_harness import dsa_uniform
from pydcop_amd.graph import FlatGraph, Params
from pydcop_amd.mgm import name_ranks

FAVORS = ("unilateral", "no", "coordinated")


class OracleMgm2:
    def __init__(self, graph: FlatGraph, params: Params = None, threshold=0.5, favor="unilateral", seed=0):
        g = graph
        self.graph = g
        self.params = params or Params()
        self.T = np.float32 if self.params.dtype == "f32" else np.float64
        self.is_max = self.params.mode == "max"
        self.threshold, self.favor, self.seed = float(threshold), favor, int(seed)
        assert favor in FAVORS
        nV = g.n_vars
        self.dom = g.dom_size.astype(np.int64)
        self.vrow = g.var_rowptr.astype(np.int64)
        self.tables = g.tables.astype(self.T)
        self.rank = name_ranks(g.var_names) if g.var_names else np.arange(nV)
        # the slot view: slot s = (variable, its k-th constraint), the table offset of v at x and the
        # other scope variables with their strides (row-major, last position contiguous)
        efac = np.repeat(np.arange(g.n_factors), np.diff(g.factor_rowptr))
        nS = len(g.var_edges)
        self.base = np.zeros(nS, dtype=np.int64)
        self.stride_v = np.zeros(nS, dtype=np.int64)
        nbs = []
        self.neigh = [[] for _ in range(nV)]
        for v in range(nV):
            seen = set()
            for s in range(self.vrow[v], self.vrow[v + 1]):
                f = int(efac[g.var_edges[s]])
                self.base[s] = g.table_off[f]
                stride, sv, lst = 1, 0, []
                for e in range(g.factor_rowptr[f + 1] - 1, g.factor_rowptr[f] - 1, -1):
                    u = int(g.edge_var[e])
                    if u == v:
                        sv += stride
                    else:
                        lst.append((u, stride))
                        seen.add(u)
                    stride *= int(self.dom[u])
                self.stride_v[s] = sv
                nbs.append(lst)
            self.neigh[v] = sorted(seen)
        J = max([len(l) for l in nbs] + [1])
        self.nbv = np.full((max(nS, 1), J), -1, dtype=np.int64)
        self.nbs = np.zeros((max(nS, 1), J), dtype=np.int64)
        for s, l in enumerate(nbs):
            for j, (u, st) in enumerate(l):
                self.nbv[s, j], self.nbs[s, j] = u, st
        self.has_nb = np.array([len(n) > 0 for n in self.neigh], dtype=bool)
        self.reset()

    # ---- sums ----------------------------------------------------------------------------------
    def _slot_sum(self, vq, xq, uq=None, yq=None, skip_u=False):
        """For every query i: sum from 0 over the constraints of vq[i], in order, of the entry with
        vq[i] at xq[i], uq[i] at yq[i] and the others at their current values; skip_u: only the
        constraints without uq[i].  Vectorised over the queries, sequential over positions."""
        T = self.T
        vq = np.asarray(vq, dtype=np.int64)
        xq = np.asarray(xq, dtype=np.int64)
        n = vq.shape[0]
        uq = np.full(n, -1, dtype=np.int64) if uq is None else np.asarray(uq, dtype=np.int64)
        yq = np.zeros(n, dtype=np.int64) if yq is None else np.asarray(yq, dtype=np.int64)
        acc = np.zeros(n, dtype=T)
        if n == 0:
            return acc
        s0 = self.vrow[vq]
        deg = self.vrow[vq + 1] - s0
        for k in range(int(deg.max()) if n else 0):
            act = k < deg
            s = np.where(act, s0 + k, 0)
            off = self.base[s] + xq * self.stride_v[s]
            has_u = np.zeros(n, dtype=bool)
            for j in range(self.nbv.shape[1]):
                w = self.nbv[s, j]
                valid = w >= 0
                is_u = valid & (w == uq)
                has_u |= is_u
                val = np.where(is_u, yq, self.cur[np.maximum(w, 0)])
                off = off + np.where(valid, val * self.nbs[s, j], 0)
            take = act & ~(skip_u & has_u)
            t = self.tables[np.where(take, off, 0)]
            acc = np.where(take, acc + t, acc).astype(T)
        return acc

    def _u(self, v, cycle, draw):
        return dsa_uniform(self.seed, int(v), int(cycle), draw)

    def _better(self, a, b):
        """`a` strictly improves on `b` in the phases that flip with the mode (1-2)"""
        return a < b if self.is_max else a > b

    # ---- state -----------------------------------------------------------------------------------
    def reset(self):
        """on_start (:460-495)"""
        g, T = self.graph, self.T
        nV = g.n_vars
        self.cur = np.zeros(nV, dtype=np.int64)
        self.cost = np.zeros(nV, dtype=T)
        self.has_cost = np.zeros(nV, dtype=np.uint8)
        self.rounds = 0
        self.pair_moves = 0          # moves of committed variables (both ends of a pair count)
        lonely = []
        for v in range(nV):
            if self.has_nb[v]:
                if g.init_idx is not None and g.init_idx[v] >= 0:
                    self.cur[v] = g.init_idx[v]
                else:
                    self.cur[v] = int(self._u(v, 0, 0) * self.dom[v])
            else:
                lonely.append(v)
        if lonely:
            vq = np.repeat(lonely, self.dom[lonely])
            xq = np.concatenate([np.arange(self.dom[v]) for v in lonely])
            c = self._slot_sum(vq, xq)
            i = 0
            for v in lonely:
                cv = c[i:i + self.dom[v]]
                i += self.dom[v]
                best_vals, best = self._best_values(cv)
                self.cur[v] = best_vals[int(self._u(v, 0, 0) * len(best_vals))]
                self.cost[v] = best
                self.has_cost[v] = 1

    def _best_values(self, costs):
        """_compute_best_value (:497-519)"""
        best, vals = None, []
        for x, c in enumerate(costs):
            if best is None or (best > c and not self.is_max) or (best < c and self.is_max):
                best, vals = c, [x]
            elif best == c:
                vals.append(x)
        return vals, best

    def run(self, n):
        for _ in range(int(n)):
            self._round()

    def _round(self):
        T = self.T
        r = self.rounds + 1
        act = np.flatnonzero(self.has_nb)
        # 1. value
        lcost = np.zeros(self.graph.n_vars, dtype=T)
        lcost[act] = self._slot_sum(act, self.cur[act])
        self.cost[act] = lcost[act]
        self.has_cost[act] = 1
        vq = np.repeat(act, self.dom[act])
        xq = np.concatenate([np.arange(self.dom[v]) for v in act]) if len(act) else np.zeros(0, dtype=np.int64)
        call = self._slot_sum(vq, xq)
        partner, offerer, pg, pv, committed = {}, set(), {}, {}, set()
        i = 0
        for v in act:
            c = call[i:i + self.dom[v]]
            i += self.dom[v]
            if self._u(v, r, 1) < self.threshold:
                offerer.add(v)
                nb = self.neigh[v]
                partner[v] = nb[int(self._u(v, r, 2) * len(nb))]
            vals, best = self._best_values(c)
            pg[v] = T(lcost[v] - best)
            if (not self.is_max and pg[v] > 0) or (self.is_max and pg[v] < 0):
                pv[v] = vals[int(self._u(v, r, 3) * len(vals))]
            else:
                pv[v] = int(self.cur[v])
        # offer tables
        offs = sorted(offerer)
        offers = {}
        if offs:
            vq, xq, uq, yq = [], [], [], []
            for v in offs:
                p = partner[v]
                X, Y = np.meshgrid(np.arange(self.dom[v]), np.arange(self.dom[p]), indexing="ij")
                vq.append(np.full(X.size, v)), xq.append(X.ravel()), uq.append(np.full(X.size, p)), yq.append(Y.ravel())
            cst = self._slot_sum(np.concatenate(vq), np.concatenate(xq), np.concatenate(uq), np.concatenate(yq))
            i = 0
            for v in offs:
                n = self.dom[v] * self.dom[partner[v]]
                c = cst[i:i + n].reshape(self.dom[v], self.dom[partner[v]])
                i += n
                ok = (lcost[v] < c) if self.is_max else (lcost[v] > c)
                offers[v] = (ok, (lcost[v] - c).astype(T))
        # 2. offer: each non-offerer over the offers aimed at it, offerers ascending
        aimed = {}
        for u in offs:
            if partner[u] not in offerer:
                aimed.setdefault(partner[u], []).append(u)
        accepted = {}
        if aimed:
            recv = sorted(aimed)
            pairs = [(v, u) for v in recv for u in aimed[v]]
            vq = np.concatenate([np.full(self.dom[v], v) for v, u in pairs])
            yq = np.concatenate([np.arange(self.dom[v]) for v, u in pairs])
            uq = np.concatenate([np.full(self.dom[v], u) for v, u in pairs])
            cc_all = self._slot_sum(vq, yq, uq, np.zeros_like(yq), skip_u=True)
            i, cc = 0, {}
            for v, u in pairs:
                cc[(v, u)] = cc_all[i:i + self.dom[v]]
                i += self.dom[v]
            for v in recv:
                best, ggs = T(0), []
                for u in aimed[v]:
                    ok, gain = offers[u]
                    d = (lcost[v] - cc[(v, u)]).astype(T)           # over own values (columns)
                    gg = (d[None, :] + gain).astype(T)               # (offerer value, own value)
                    ggs.append((u, ok, gg))
                    if ok.any():
                        ext = gg[ok].min() if self.is_max else gg[ok].max()
                        if self._better(ext, best):
                            best = ext
                n_best = sum(int((ok & (gg == best)).sum()) for _, ok, gg in ggs)
                commit = False
                if best == 0 or n_best == 0:
                    commit = False
                elif self._better(best, pg[v]):
                    commit = True
                elif best == pg[v]:
                    if self.favor == "coordinated":
                        commit = True
                    elif self.favor == "no" and self._u(v, r, 4) > 0.5:
                        commit = True
                if commit:
                    k = int(self._u(v, r, 5) * n_best)
                    for u, ok, gg in ggs:
                        xs, ys = np.nonzero(ok & (gg == best))      # row-major: offerer value, own value
                        if k < len(xs):
                            pv[v], pg[v] = int(ys[k]), T(best)
                            accepted[u] = (int(xs[k]), T(best))
                            partner[v] = u
                            committed.add(v)
                            break
                        k -= len(xs)
        # 3. answer
        for u in offs:
            if u in accepted:
                pv[u], pg[u] = accepted[u]
                committed.add(u)

        # 4. gain, 5. go
        def can_move(a, excl):
            gains = [pg[w] for w in self.neigh[a] if w != excl]
            return not gains or pg[a] > max(gains)

        for v in act:
            if pg[v] == 0:
                continue
            if v in committed:
                move = can_move(v, partner[v]) and can_move(partner[v], v)
            else:
                mx = max(pg[w] for w in self.neigh[v])
                if pg[v] > mx:
                    move = True
                elif pg[v] == mx:
                    ties = [self.rank[w] for w in self.neigh[v] if pg[w] == mx] + [self.rank[v]]
                    move = min(ties) == self.rank[v]
                else:
                    move = False
            if move:
                self.cur[v] = pv[v]
                self.cost[v] = T(lcost[v] - pg[v])
                self.pair_moves += v in committed
        self.rounds += 1

    @property
    def cycle_count(self):
        return self.rounds

    def state(self):
        return {"idx": self.cur.astype(np.int32), "cost": self.cost.astype(np.float64),
                "has_cost": self.has_cost.copy()}

    def assignment(self):
        s = self.state()
        return s["idx"], s["cost"]

    def eval_cost(self, idx=None, infinity=float("inf")):
        """DCOP.solution_cost (pydcop/dcop/dcop.py:308-367): constraints and variable costs."""
        g = self.graph
        idx = self.cur if idx is None else np.asarray(idx)
        soft, hard = 0.0, 0
        for f in range(g.n_factors):
            lin = 0
            for e in range(g.factor_rowptr[f], g.factor_rowptr[f + 1]):
                u = g.edge_var[e]
                lin = lin * int(g.dom_size[u]) + int(idx[u])
            x = float(g.tables[g.table_off[f] + lin])
            if x != infinity:
                soft += x
            else:
                hard += 1
        ev = g.eval_var_cost if g.eval_var_cost is not None else g.var_cost
        off = g.cost_off
        for v in range(g.n_vars):
            x = float(ev[off[v] + idx[v]])
            if x != infinity:
                soft += x
            else:
                hard += 1
        return soft, hard

    def close(self):
        pass
