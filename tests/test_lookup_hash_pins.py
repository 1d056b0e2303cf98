"""CPU: tests/lookup_edge_cases.py chooses its adversarial keys with a Python restatement of the multiplicity table's hash and capacity
rule.  If csrc/rowprog.hip changes either, those keys silently stop colliding and the cases lose their teeth: fail here instead."""
import os
import re

import numpy as np

from conftest import ROOT
from lookup_edge_cases import HASH_MUL, HASH_SEED, HASH_SHIFT, fe_hash, last_slot_keys, rand_words, table_capacity


def _source():
    with open(os.path.join(ROOT, "sirius_amd", "csrc", "rowprog.hip")) as f:
        return f.read()


def _body(src, head):
    """the brace-balanced body of the function whose definition starts with `head`"""
    start = src.index(head)
    i = src.index("{", start)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        j += 1
        if depth == 0:
            return src[i:j]


def test_fe_hash_source_matches_the_restatement():
    body = re.sub(r"\s+", " ", _body(_source(), "uint32_t fe_hash(const fe_t &x)"))
    assert f"uint32_t h = 0x{HASH_SEED:08X}u;" in body
    assert "for (int i = 0; i < 8; ++i) { h ^= x.v[i]; h *= 0x%08Xu; h ^= h >> %d; }" % (HASH_MUL, HASH_SHIFT) in body
    assert (HASH_SEED, HASH_MUL, HASH_SHIFT) == (0x9E3779B9, 0x85EBCA6B, 15)
    assert body.count("0x") == 2 and body.count(">>") == 1            # nothing else is mixed in


def test_probe_starts_at_hash_and_mask():
    src = _source()
    for head in ("void k_m_insert(", "void k_m_count(", "void k_m_emit("):
        body = _body(src, head)
        assert "uint32_t s = fe_hash(key) & mask;" in body and "s = (s + 1) & mask;" in body, head


def test_capacity_rule_source_matches_the_restatement():
    body = re.sub(r"\s+", " ", _body(_source(), "int lookup_coeff_1(Structure *S"))
    assert "uint32_t cap = 2; while (cap < 2 * n) cap <<= 1;" in body
    assert "cap - 1);" in body and "cap - 1, ms[i]);" in body            # the kernels get mask = cap - 1
    assert [table_capacity(r) for r in (0, 1, 2, 3, 32, 33, 1024)] == [2, 2, 4, 8, 64, 128, 2048]


def test_fe_hash_vectorised_equals_scalar():
    words = rand_words(np.random.default_rng(3), 64)
    words[0] = 0
    words[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for w, got in zip(words, fe_hash(words)):
        v = sum(int(x) << (64 * i) for i, x in enumerate(w))
        h = HASH_SEED
        for i in range(8):
            h ^= (v >> (32 * i)) & 0xFFFFFFFF
            h = (h * HASH_MUL) & 0xFFFFFFFF
            h ^= h >> HASH_SHIFT
        assert int(got) == h


def test_collision_key_search_finds_enough_keys():
    """Hard requirement of collision_case (an assert inside last_slot_keys, never a skip): rows + rows / 2 keys in the last slot."""
    for k in (5, 10):
        rows = 1 << k
        keys = last_slot_keys(k)
        cap = table_capacity(rows)
        assert cap == 2 * rows and keys.shape == (rows + rows // 2, 4)
        assert np.all((fe_hash(keys) & np.uint64(cap - 1)) == np.uint64(cap - 1))
