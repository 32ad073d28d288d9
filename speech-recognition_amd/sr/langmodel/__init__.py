# -*- coding: utf-8 -*-
"""`sr.langmodel` -- lexical-tree spell check and bigram language model, MI355X-native.

Same importable names as the reference package (sr/langmodel/__init__.py): LexNode, append_lex_node,
lextree_from_words, get_nodes, text_viterbi, SpellChecker; plus text_viterbi_batch and BigramModel (langmodel.py, an empty
file in the reference: word-to-word costs for `ContinuousDecoder(grammar="bigram")`).  The tree is built on the host;
text_viterbi's dynamic program runs in HIP kernels through libgmmhmm.so (gh_text_viterbi), with no CPU fallback.
"""
from .langmodel import *  # noqa: F401,F403
from .lextree import *  # noqa: F401,F403
from .spellchecker import *  # noqa: F401,F403
