# -*- coding: utf-8 -*-
"""sr.langmodel on the GPU (gh_text_viterbi, csrc/gh_lextree.hip): the reference's text_viterbi results (G19) exactly,
random trees / distances / Unicode against the numpy restatement, batches against single calls, both cost forms."""
import numpy as np
import pytest

from conftest import load_golden
import langmodel_ref as LR
from test_langmodel_host import DIST, g19_trees

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trees():
    return g19_trees(load_golden("G18_lextree"))


def test_device_equals_the_reference(trees):
    from sr.langmodel import text_viterbi
    g = load_golden("G19_text_viterbi")
    for tree, x, dist, cost, matched in zip(g["tree"], g["x"], g["dist"], g["cost"], g["matched"]):
        c, s = text_viterbi(str(x), trees[str(tree)], DIST[str(dist)])
        assert type(c) is np.float64
        assert (c, s) == (cost, str(matched)), (tree, x)


def random_case(rng):
    """A hand-built tree (multi-character and Unicode values, the root sometimes a word end), a string and an
    integer distance drawn as a table."""
    from sr.langmodel import LexNode, append_lex_node
    pool = ["a", "b", "ab", "é", "ß", "日本", "z", " ", "xy"]
    root = LexNode("*")
    root.property = 2 if rng.random() < 0.1 else 1
    nodes = [root]
    for _ in range(int(rng.integers(1, 40))):
        n = LexNode(str(rng.choice(pool)))
        n.property = 2 if rng.random() < 0.4 else 0
        append_lex_node(nodes[int(rng.integers(len(nodes)))], n)
        nodes.append(n)
    nodes[-1].property = 2
    chars = "ab*é日z ßq"
    x = "".join(rng.choice(list(chars), size=int(rng.integers(1, 30))))
    table = {(c, v): int(rng.integers(0, 5)) for c in chars for v in pool + ["*"]}
    return root, x, lambda a, b: table[(a, b)]


def test_random_cases_equal_the_restatement():
    from sr.langmodel import text_viterbi
    from sr.langmodel.spellchecker import FlatTree
    rng = np.random.default_rng(2024)
    for i in range(320):
        tree, x, dist = random_case(rng)
        got = text_viterbi(x, tree, dist)
        assert got == LR.text_viterbi(x, FlatTree(tree), dist), (i, x)


def test_batch_equals_single_calls_and_chunks(trees, monkeypatch):
    from sr.langmodel import text_viterbi, text_viterbi_batch
    from sr.recognition import _hip
    rng = np.random.default_rng(7)
    strings = ["".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz '"), size=int(rng.integers(1, 25)))) for _ in range(60)]
    one = [text_viterbi(x, trees["dict1"]) for x in strings]
    costs, matched = text_viterbi_batch(strings, trees["dict1"])
    assert list(zip(costs, matched)) == one
    assert _hip.default_context().last_chunks == 1
    monkeypatch.setenv("GMMHMM_SCRATCH_BUDGET", "2M")
    costs2, matched2 = text_viterbi_batch(strings, trees["dict1"])
    assert _hip.default_context().last_chunks > 3
    np.testing.assert_array_equal(costs2, costs)
    assert matched2 == matched


def test_lds16_and_32bit_forms_agree(trees, monkeypatch):
    from sr.langmodel import text_viterbi_batch
    from sr.langmodel.spellchecker import FlatTree
    rng = np.random.default_rng(11)
    strings = ["".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), size=int(rng.integers(1, 40)))) for _ in range(40)]
    for key in ("dict1", "s0", "s3"):
        a = text_viterbi_batch(strings, trees[key])
        monkeypatch.setenv("GMMHMM_LEXTREE_FORM", "32")
        b = text_viterbi_batch(strings, trees[key])
        monkeypatch.delenv("GMMHMM_LEXTREE_FORM")
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
    # costs beyond 16 bits pick the 32-bit form by themselves
    big = lambda a, b: 0 if a == b else 40000
    x = strings[0]
    c, s = text_viterbi_batch([x], trees["s1"], big)
    rc, rs = LR.text_viterbi(x, FlatTree(trees["s1"]), big)
    assert (c[0], s[0]) == (rc, rs) and rc > 65535


def test_costs_beyond_32_bits_are_unsupported(trees):
    from sr.langmodel import text_viterbi
    from sr.recognition import _hip
    with pytest.raises(_hip.BackendError):
        text_viterbi("abc", trees["s0"], lambda a, b: 0 if a == b else 2 ** 31)


def test_spellchecker(trees):
    from sr.langmodel import SpellChecker, text_viterbi
    words = [str(w) for w in load_golden("G18_lextree")["words0"]]
    sc = SpellChecker(beam=5)
    d = list(words)
    sc.fit(d)
    assert sc.dictionary is d and d == words and sc.beam == 5
    texts = ["helo", "wrld", "spel chek", "a"]
    assert sc.spell_check(texts[0]) == text_viterbi(texts[0], trees["dict1"])[1]
    assert sc.spell_check(texts) == [text_viterbi(t, trees["dict1"])[1] for t in texts]


def test_create_rejects_bad_trees():
    from sr.recognition import _hip
    ctx = _hip.default_context()
    ok = dict(parent=[-1, 0, 1, -1], val_code=[0, 1, 2, 3], n_val=4, word_ends=[3, 2], depth=2)
    _hip.LexTree(ctx, **ok).close()
    for bad in (dict(ok, parent=[-1, 7, 1, -1]),          # parent out of range
                dict(ok, parent=[-1, 2, 1, -1]),          # cycle 1 <-> 2
                dict(ok, word_ends=[3, 9]),               # word end out of range
                dict(ok, word_ends=[2, 1]),               # the space row must come first
                dict(ok, val_code=[0, 1, 5, 3])):
        with pytest.raises(_hip.BackendError):
            _hip.LexTree(ctx, **bad)
