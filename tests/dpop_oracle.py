"""DPOP restated in numpy on a FlatGraph and a pseudo-tree (TEST ORACLE; pinned against the reference's own
DpopAlgo objects by tests/test_dpop_oracle_vs_reference.py).

The reference (pydcop/algorithms/dpop.py:174-441, pydcop/dcop/relations.py:1554-1591, 1672-1756):
  * a constraint belongs to the lowest node of its scope (dpop.py:188-199), in the node's constraint order;
  * node v joins its cost vector (dims [v], dpop.py:204-210), then each child's UTIL in children order, then
    its constraints: `join` lists u1's dimensions first, then u2's new ones, and adds entry by entry, so the
    joined entry is (((cost_v[d] + U_c1) + U_c2) + ... + r_1) + ...; a broadcast add does the same IEEE add
    per entry;
  * `projection` takes, per separator assignment, the first optimum over v's domain under a strict compare
    (the VALUE of a minimum does not depend on which minimiser is kept: `.min(axis=0)`);
  * VALUE: the joined table sliced at the separator's chosen values, first optimum; the node reports the
    joined value there (dpop.py:417-441; roots: dpop.py:352-367, isolated variables: dpop.py:252-274).
The joined tables are not kept: VALUE gathers the same terms in the same order at the chosen indices."""
import numpy as np


class OracleDpop:
    def __init__(self, graph, params=None, tree=None):
        from pydcop_amd.dpop import build_pseudotree
        from pydcop_amd.graph import Params
        self.graph = g = graph
        self.params = params or Params()
        self.T = np.float32 if self.params.dtype == "f32" else np.float64
        self.is_max = self.params.mode == "max"
        self.parent, crow, cidx = (np.asarray(a) for a in (build_pseudotree(g) if tree is None else tree))
        n = g.n_vars
        self.children = [[int(c) for c in cidx[crow[v]:crow[v + 1]]] for v in range(n)]
        self.depth = np.zeros(n, dtype=np.int64)
        self.order = []                                        # pre-order: parents before children
        stack = [r for r in range(n - 1, -1, -1) if self.parent[r] < 0]
        while stack:
            v = stack.pop()
            self.order.append(v)
            for c in reversed(self.children[v]):
                self.depth[c] = self.depth[v] + 1
                stack.append(c)
        assert len(self.order) == n, "not a tree"
        # constraints: to the deepest variable of the scope, in that variable's var_edges order
        fac_of_edge = np.repeat(np.arange(g.n_factors), np.diff(g.factor_rowptr))
        self.scope = [[int(u) for u in g.edge_var[g.factor_rowptr[f]:g.factor_rowptr[f + 1]]] for f in range(g.n_factors)]
        owner = [max(s, key=lambda u: self.depth[u]) for s in self.scope]
        self.cons = [[] for _ in range(n)]
        for v in range(n):
            for e in g.var_edges[g.var_rowptr[v]:g.var_rowptr[v + 1]]:
                f = int(fac_of_edge[e])
                if owner[f] == v and f not in self.cons[v]:
                    self.cons[v].append(f)
        coff = g.cost_off
        self.cost_vec = [g.var_cost[coff[v]:coff[v + 1]].astype(self.T) for v in range(n)]
        self.util = {}       # v -> (dims, table)
        self.idx = np.zeros(n, dtype=np.int32)
        self.cost = np.zeros(n, dtype=np.float64)

    def _table(self, f):
        g = self.graph
        return g.tables[g.table_off[f]:g.table_off[f + 1]].astype(self.T).reshape([int(g.dom_size[u]) for u in self.scope[f]])

    def _terms(self, v):
        """(dims, table) of every term of v's join after its cost vector, in the reference's order"""
        return [self.util[c] for c in self.children[v]] + [(self.scope[f], self._table(f)) for f in self.cons[v]]

    @staticmethod
    def _aligned(table, dims, out_dims):
        """`table` over `dims` (a variable may repeat: the diagonal) as a broadcastable view over out_dims"""
        uniq = []
        for u in dims:
            if u not in uniq:
                uniq.append(u)
        letters = {u: chr(ord("a") + i) if i < 26 else chr(ord("A") + i - 26) for i, u in enumerate(uniq)}
        if len(uniq) != len(dims):
            table = np.einsum("".join(letters[u] for u in dims) + "->" + "".join(letters[u] for u in uniq), table)
        present = [u for u in out_dims if u in letters]
        t = np.transpose(table, [uniq.index(u) for u in present])
        return t.reshape([t.shape[present.index(u)] if u in letters else 1 for u in out_dims])

    def solve(self):
        g = self.graph
        for v in reversed(self.order):                         # UTIL: children before parents
            if self.parent[v] < 0:
                continue
            terms = self._terms(v)
            dims = [v]
            for d2, _ in terms:
                for u in d2:
                    if u not in dims:
                        dims.append(u)
            joined = self._aligned(self.cost_vec[v], [v], dims)
            for d2, t in terms:
                joined = joined + self._aligned(t, d2, dims)
            joined = np.broadcast_to(joined, [int(g.dom_size[u]) for u in dims])
            self.util[v] = (dims[1:], joined.max(axis=0) if self.is_max else joined.min(axis=0))
        for v in self.order:                                   # VALUE: parents before children
            vec = self.cost_vec[v]
            for d2, t in self._terms(v):
                sl = tuple(slice(None) if u == v else int(self.idx[u]) for u in d2)
                part = t[sl]
                if part.ndim > 1:                              # (v twice in a scope)
                    part = np.einsum("i" * part.ndim + "->i", part)
                vec = vec + part
            d = int(np.argmax(vec) if self.is_max else np.argmin(vec))   # (the first optimum)
            self.idx[v], self.cost[v] = d, float(vec[d])
        return self

    def state(self):
        return {"idx": self.idx.copy(), "cost": self.cost.copy()}

    def stats(self):
        ent = [int(t.size) for _, t in self.util.values()]
        return {"components": int((self.parent < 0).sum()), "depth": int(self.depth.max()) if len(self.depth) else 0,
                "widest_separator": max([len(d) for d, _ in self.util.values()] or [0]),
                "widest_util_entries": max(ent or [0]), "total_entries": sum(ent),
                "bytes": sum(ent) * np.dtype(self.T).itemsize}

    def eval_cost(self, idx=None):
        g = self.graph
        idx = self.idx if idx is None else idx
        total = 0.0
        for f, s in enumerate(self.scope):
            total += float(g.tables[g.table_off[f]:g.table_off[f + 1]].reshape([int(g.dom_size[u]) for u in s])[tuple(int(idx[u]) for u in s)])
        ev = g.eval_var_cost if g.eval_var_cost is not None else g.var_cost
        return total + float(ev[g.cost_off[:-1] + idx].sum())
