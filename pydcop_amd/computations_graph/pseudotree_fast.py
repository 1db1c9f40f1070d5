"""pseudotree_fast -- the reference's DFS pseudo-tree, built without recursion in O(E * degree).

`pydcop.computations_graph.pseudotree.build_computation_graph` (pseudotree.py:472-539) finds every
node's neighbours by scanning all constraints and all nodes (`_find_neighbors_relations`, O(V*C*V)),
walks the tree recursively (two Python frames per level: a 1 024-variable strip needs a raised recursion
limit) and tests `in token` on a list.  This module returns an EQUAL graph -- the reference's own
`ComputationPseudoTree`, `PseudoTreeNode` and `PseudoTreeLink` classes, the same roots, parents,
children order, pseudo-parents and pseudo-children order, the same constraints per node -- from
`pydcop_amd.dpop.dfs_pseudotree`, which restates the heuristic with mark arrays.
Drop-in: an algorithm module with `GRAPH_TYPE = "pseudotree_fast"`.
"""
from typing import Iterable

from pydcop.computations_graph.pseudotree import (ComputationPseudoTree, PseudoTreeLink,  # noqa: F401
                                                   PseudoTreeNode, _BuildingNode, get_dfs_relations)
from pydcop.dcop.dcop import DCOP
from pydcop.dcop.objects import Variable
from pydcop.dcop.relations import Constraint

from pydcop_amd.dpop import dfs_pseudotree, neighbor_lists_of_scopes

GRAPH_NODE_TYPES = ("PseudoTreeComputation",)


def build_computation_graph(dcop: DCOP = None, variables: Iterable[Variable] = None,
                            constraints: Iterable[Constraint] = None) -> ComputationPseudoTree:
    """Same contract as pseudotree.build_computation_graph (pseudotree.py:472-539)."""
    if dcop is not None:
        if constraints or variables is not None:
            raise ValueError("Cannot use both dcop and constraints / variables parameters")
        variables = dcop.variables.values()
        constraints = dcop.constraints.values()
    elif constraints is None or variables is None:
        raise ValueError("Constraints AND variables parameters must be provided when not "
                         "building the graph from a dcop")
    variables, constraints = list(variables), list(constraints)
    index = {}
    for i, v in enumerate(variables):
        index.setdefault(v.name, i)
    scopes = [[index[v.name] for v in c.dimensions if v.name in index] for c in constraints]
    roots, parent, children, pseudo_parents, pseudo_children = dfs_pseudotree(
        neighbor_lists_of_scopes(len(variables), scopes))
    nodes = [_BuildingNode(v) for v in variables]
    for f, scope in enumerate(scopes):          # a node's relations: its constraints in their order
        for i in dict.fromkeys(scope):
            nodes[i].relations.append(constraints[f])
    for i, n in enumerate(nodes):
        n.parent = nodes[parent[i]] if parent[i] >= 0 else None
        n.root = parent[i] < 0
        n.children = [nodes[c] for c in children[i]]
        n.pseudo_parents = [nodes[c] for c in pseudo_parents[i]]
        n.pseudo_children = [nodes[c] for c in pseudo_children[i]]
    return ComputationPseudoTree([nodes[r] for r in roots])
