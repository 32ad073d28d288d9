# -*- coding: utf-8 -*-
"""Spell check against a lexical tree (sr/langmodel/spellchecker.py): text_viterbi's dynamic program runs on the GPU
(gh_text_viterbi, csrc/gh_lextree.hip); the tree is flattened and the distances are tabulated here."""
import math
import numbers

import numpy as np

from .lextree import LexNode

__all__ = ["get_nodes", "text_viterbi", "text_viterbi_batch", "SpellChecker"]


def get_nodes(node_list, lexnode):
    """Append `lexnode` and its subtree to node_list in preorder."""
    node_list.append(lexnode)
    for c in lexnode.children:
        get_nodes(node_list, c)


def _mismatch(a, b):
    return int(a != b)


class FlatTree:
    """A tree as rows: preorder (row 0 the root), then the extra space row R-1.
        vals, prop    each row's value and property (the space row: ' ', 0)
        parent        [R] int32, -1 for the root and the space row (the reference's `transitions`, child -> parent)
        depth         [R] int32 (the space row: 0)
        word_ends     [space row] + the rows of property 2 in preorder (the reference's `word_ends`)
    Built in O(R) through an id() map; a node reachable twice (shared between parents, or a cycle) is a ValueError."""

    def __init__(self, lextree):
        if type(lextree) is not LexNode:
            raise TypeError("text_viterbi: the tree must be a LexNode, not %s" % type(lextree).__name__)
        rows = {}
        vals, prop, parent, depth = [], [], [], []
        stack = [(lextree, -1, 0)]
        while stack:
            node, p, d = stack.pop()
            if id(node) in rows:
                raise ValueError("text_viterbi: node %r is reachable twice (shared between parents, or a cycle)" % (node.val,))
            rows[id(node)] = r = len(vals)
            vals.append(node.val)
            prop.append(node.property)
            parent.append(p)
            depth.append(d)
            for child in reversed(node.children):
                stack.append((child, r, d + 1))
        vals.append(" ")
        prop.append(0)
        parent.append(-1)
        depth.append(0)
        self.vals = vals
        self.R = len(vals)
        self.prop = np.array([p == 2 for p in prop])
        self.parent = np.array(parent, dtype=np.int32)
        self.depth = np.array(depth, dtype=np.int32)
        self.max_depth = int(self.depth.max())
        self.word_ends = np.concatenate([[self.R - 1], np.nonzero(self.prop)[0]]).astype(np.int32)
        if len(self.word_ends) < 2:
            raise ValueError("text_viterbi: the tree has no word end (no node of property 2)")
        self.val_index = {}
        for v in vals:
            self.val_index.setdefault(v, len(self.val_index))
        self.val_code = np.array([self.val_index[v] for v in vals], dtype=np.int32)


def _cost_value(v, a, b):
    """A dist_fun result as a Python int: non-negative, finite and integral, else ValueError."""
    if isinstance(v, numbers.Integral):
        iv = int(v)
    elif isinstance(v, numbers.Real) and math.isfinite(float(v)) and float(v).is_integer():
        iv = int(v)
    else:
        raise ValueError("text_viterbi: dist_fun(%r, %r) = %r is not a non-negative finite integer" % (a, b, v))
    if iv < 0:
        raise ValueError("text_viterbi: dist_fun(%r, %r) = %r is negative" % (a, b, v))
    return iv


def _encode(strings, flat, dist_fun):
    """Codes of '*' + x for every string (offsets, codes) and the integer table dist[x character, node value]."""
    chars = {}
    offsets = np.zeros(len(strings) + 1, dtype=np.int64)
    codes = []
    for i, x in enumerate(strings):
        if not isinstance(x, str):
            raise TypeError("text_viterbi: x must be a str, not %s" % type(x).__name__)
        if len(x) == 0:
            raise ValueError("text_viterbi: x is empty (the reference's back-trace never ends on it)")
        for ch in "*" + x:
            codes.append(chars.setdefault(ch, len(chars)))
        offsets[i + 1] = len(codes)
    vals = list(flat.val_index)
    table = np.empty((max(len(chars), 1), len(vals)), dtype=np.int64)
    for ch, i in chars.items():
        for j, v in enumerate(vals):
            table[i, j] = _cost_value(dist_fun(ch, v), ch, v)
    return offsets, np.array(codes, dtype=np.int32), table


class _DeviceTree:
    """A FlatTree resident on a GPU (one upload)."""

    def __init__(self, flat, ctx=None):
        from ..recognition import _hip
        self.flat = flat
        ctx = ctx or _hip.default_context()
        self.tree = _hip.LexTree(ctx, flat.parent, flat.val_code, len(flat.val_index), flat.word_ends, flat.max_depth)

    def run(self, encoded):
        """(costs, matched strings) of strings _encode()d against this tree."""
        flat = self.flat
        best, paths = self.tree.viterbi(*encoded)
        out = []
        for rows in paths:
            s = flat.vals[rows[0]]
            for r in rows[1:]:
                s += flat.vals[r]
            out.append(s[::-1])
        return best.astype(np.float64), out


def text_viterbi(x, lextree, dist_fun=_mismatch):
    """(cost, matched string) of `x` against the lexical tree -- the reference's result exactly.
    dist_fun(character of '*' + x, node value) must give non-negative finite integers (else ValueError: the kernels
    compute in integers); an empty x is a ValueError (the reference does not return on it)."""
    costs, strings = text_viterbi_batch([x], lextree, dist_fun)
    return costs[0], strings[0]


def text_viterbi_batch(strings, lextree, dist_fun=_mismatch):
    """text_viterbi of every string of `strings` against one tree: one upload of the tree, one launch per chunk of the
    decision memory budget.  -> (costs float64 [B], list of B matched strings)."""
    flat = FlatTree(lextree)
    strings = list(strings)
    if not strings:
        return np.zeros(0), []
    encoded = _encode(strings, flat, dist_fun)     # (ValueError / TypeError before the GPU is touched)
    return _DeviceTree(flat).run(encoded)


class SpellChecker:
    """Spell check against a dictionary.  `beam` is stored and not used (as in the reference: no pruning)."""

    def __init__(self, beam):
        self.dictionary = None
        self.beam = beam
        self.lextree = None
        self._device = None

    def fit(self, dictionary):
        """Keep `dictionary` (the object itself) and build its lexical tree from a copy (lextree_from_words pads and
        shortens the list it is given), resident on the GPU."""
        from .lextree import lextree_from_words
        self.dictionary = dictionary
        self.lextree = lextree_from_words(list(dictionary))
        self._device = _DeviceTree(FlatTree(self.lextree))

    def spell_check(self, text, dist_fun=_mismatch):
        """text_viterbi(text, tree)[1]; a list of strings gives a list, run as one batch."""
        if self._device is None:
            raise RuntimeError("SpellChecker.spell_check before fit")
        if isinstance(text, str):
            return self._device.run(_encode([text], self._device.flat, dist_fun))[1][0]
        text = list(text)
        if not text:
            return []
        return self._device.run(_encode(text, self._device.flat, dist_fun))[1]
