# -*- coding: utf-8 -*-
"""Lexical (prefix) tree of a word list, node for node as the reference builds it (sr/langmodel/lextree.py)."""
__all__ = ["LexNode", "append_lex_node", "lextree_from_words"]


class LexNode:
    """One character of the tree.  property: 0 an inner node, 1 the root, 2 the last character of a word."""

    def __init__(self, val):
        self.val = val
        self.children = []
        self.property = 0

    def pretty_str(self, level=0):
        """The subtree, one repr per line, indented by depth.  (The reference recurses through `__str__` here, which
        takes no level and raises; this recurses through pretty_str.)"""
        lines = "\t" * level + repr(self.val) + "\n"
        for child in self.children:
            lines += child.pretty_str(level + 1)
        return lines

    def __str__(self):
        return self.val

    def get_max_level(self, level=0):
        """Depth of the deepest node below this one (this one at `level`)."""
        if not self.children:
            return level
        return max(child.get_max_level(level=level + 1) for child in self.children)


def append_lex_node(parent, child):
    assert type(parent) is LexNode and type(child) is LexNode
    parent.children.append(child)


def _grow(node, words, i, width):
    """Children of `node` for the padded `words` that share its prefix, from character position i."""
    if i >= width:
        return
    # A word whose character i is its last gets a leaf of its own (property 2) and leaves `words`.  The removal happens
    # while the list is walked by index, so the word after each removed one is not looked at in this pass -- as in the
    # reference, whose `for w in words: ... words.remove(w)` does the same.  remove() drops the FIRST equal entry.
    k = 0
    while k < len(words):
        w = words[k]
        if i == width - 1 or w[i + 1] == " ":
            leaf = LexNode(w[i])
            leaf.property = 2
            append_lex_node(node, leaf)
            words.remove(w)
        k += 1
    # the remaining words by their character i, characters in order of first appearance
    groups = {}
    for w in words:
        groups.setdefault(w[i], []).append(w)
    for ch, members in groups.items():
        child = LexNode(ch)
        append_lex_node(node, child)
        _grow(child, members, i + 1, width)


def lextree_from_words(words):
    """Build the lexical tree of `words` (root '*', property 1).  Like the reference, the caller's list is padded with
    ' ' to the longest word IN PLACE, and the words of one character are removed from it (see _grow)."""
    root = LexNode("*")
    root.property = 1
    width = max([len(w) for w in words])
    for n in range(len(words)):
        words[n] = words[n].ljust(width, " ")
    _grow(root, words, 0, width)
    return root
