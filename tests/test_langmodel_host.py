# -*- coding: utf-8 -*-
"""sr.langmodel on the host: the lexical tree node for node against the reference (G18), the flattening, the numpy
restatement of text_viterbi against the reference's results (G19), and the errors raised before any GPU work."""
import numpy as np
import pytest

from conftest import has_gpu, load_golden
import langmodel_ref as LR


def dist_vowel3(a, b):
    """G19's custom integer distance (tools/make_goldens.py)."""
    if a == b:
        return 0
    return 1 if (a in "aeiou" and b in "aeiou") else 3


DIST = {"mismatch": lambda a, b: int(a != b), "vowel3": dist_vowel3}


@pytest.fixture(scope="module")
def g18():
    return load_golden("G18_lextree")


@pytest.fixture(scope="module")
def g19():
    return load_golden("G19_text_viterbi")


def g19_trees(g18):
    """The trees G19 ran on: s0..s4 = G18's small lists 1..5, dict1 = G18's list 0."""
    from sr.langmodel import lextree_from_words
    trees = {"s%d" % t: lextree_from_words(list(g18["words%d" % (t + 1)])) for t in range(5)}
    trees["dict1"] = lextree_from_words(list(g18["words0"]))
    return trees


def test_star_export_surface():
    import sr.langmodel as L
    ns = {}
    exec("from sr.langmodel import *", ns)
    for name in ("LexNode", "append_lex_node", "lextree_from_words", "get_nodes", "text_viterbi", "SpellChecker",
                 "text_viterbi_batch"):
        assert ns[name] is getattr(L, name)
    import sr
    assert not hasattr(sr, "langmodel") or sr.langmodel is L   # (sr/__init__.py does not import it)


def test_trees_match_the_reference_node_for_node(g18):
    from sr.langmodel import lextree_from_words, get_nodes
    from sr.langmodel.spellchecker import FlatTree
    for i in range(int(g18["n"])):
        words = [str(w) for w in g18["words%d" % i]]
        tree = lextree_from_words(words)
        assert words == [str(w) for w in g18["after%d" % i]], i      # the caller's list, padded and shortened
        nodes = []
        get_nodes(nodes, tree)
        assert [n.val for n in nodes] == list(g18["vals%d" % i]), i
        assert [n.property for n in nodes] == list(g18["prop%d" % i]), i
        assert tree.get_max_level() == int(g18["max_level%d" % i])
        flat = FlatTree(tree)
        np.testing.assert_array_equal(flat.parent, g18["parent%d" % i])
        np.testing.assert_array_equal(flat.word_ends, g18["word_ends%d" % i])
        assert flat.vals == list(g18["vals%d" % i]) + [" "]


def test_dict1_tree_shape(g18):
    assert len(g18["vals0"]) == 27590 and int((g18["vals0"] == " ").sum()) == 39
    assert len(g18["words0"]) == 6249 and len(g18["after0"]) == 6245 and int(g18["max_level0"]) == 20


def test_restatement_reproduces_the_reference(g18, g19):
    from sr.langmodel.spellchecker import FlatTree
    flats = {k: FlatTree(t) for k, t in g19_trees(g18).items()}
    for tree, x, dist, cost, matched in zip(g19["tree"], g19["x"], g19["dist"], g19["cost"], g19["matched"]):
        c, s = LR.text_viterbi(str(x), flats[str(tree)], DIST[str(dist)])
        assert (c, s) == (cost, str(matched)), (tree, x)
    assert max(len(str(x)) for x in g19["x"]) >= 1900 and min(len(str(x)) for x in g19["x"]) == 1


def test_pretty_str_and_str():
    from sr.langmodel import LexNode, append_lex_node
    root = LexNode("*")
    a = LexNode("a")
    append_lex_node(root, a)
    append_lex_node(a, LexNode("b"))
    assert root.pretty_str() == "'*'\n\t'a'\n\t\t'b'\n"
    assert str(a) == "a" and root.get_max_level() == 2 and a.get_max_level(level=1) == 2
    with pytest.raises(AssertionError):
        append_lex_node(root, "c")


def test_value_errors_before_the_gpu():
    from sr.langmodel import LexNode, append_lex_node, lextree_from_words, text_viterbi, text_viterbi_batch
    tree = lextree_from_words(["ab", "ac", "b"])
    with pytest.raises(ValueError):
        text_viterbi("", tree)
    with pytest.raises(ValueError):
        text_viterbi_batch(["a", ""], tree)
    for bad in (0.5, -1, float("inf"), float("nan"), "1", None):
        with pytest.raises(ValueError):
            text_viterbi("ab", tree, dist_fun=lambda a, b, v=bad: v if a != b else 0)
    root = LexNode("*")
    shared = LexNode("x")
    shared.property = 2
    p, q = LexNode("p"), LexNode("q")
    for n in (p, q):
        append_lex_node(root, n)
        append_lex_node(n, shared)
    with pytest.raises(ValueError):
        text_viterbi("px", root)
    cyc = LexNode("*")
    c1 = LexNode("c")
    c1.property = 2
    append_lex_node(cyc, c1)
    append_lex_node(c1, cyc)
    with pytest.raises(ValueError):
        text_viterbi("c", cyc)
    with pytest.raises(ValueError):      # no word end at all (the reference's argmin of an empty list)
        text_viterbi("a", LexNode("*"))


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_text_viterbi_without_gpu_is_a_backend_error(built_library):
    from sr.recognition import _hip
    from sr.langmodel import lextree_from_words, text_viterbi, SpellChecker
    with pytest.raises(_hip.BackendError):
        text_viterbi("ab", lextree_from_words(["ab", "ba"]))
    with pytest.raises(_hip.BackendError):
        SpellChecker(3).fit(["ab", "ba"])
