"""The pure-numpy half of the staging helper (confidence_bootstrapping_amd/staging.py): where every host array of a ragged-batch launch
lands in the one buffer of 4-byte words that is uploaded.  No GPU."""
import itertools

import numpy as np
import pytest

from confidence_bootstrapping_amd.staging import layout, ptr


def _arrays():
    rng = np.random.default_rng(0)
    return {
        "lig_ptr": ptr([3, 0, 5]),                                                     # int32, 4 words
        "pos": rng.standard_normal((7, 3)).astype(np.float32),                         # 21 words: odd
        "tor": rng.uniform(-np.pi, np.pi, 5),                                          # float64 behind an odd number of 4-byte words
        "mask_bits": rng.integers(0, 2 ** 32, 3, dtype=np.uint64).astype(np.uint32),   # 3 words: odd
        "no_bonds": np.zeros((0, 2), dtype=np.int32),
        "tables": rng.integers(0, 2 ** 63, 3, dtype=np.uint64) | np.uint64(1 << 63),   # pointer-like, top bit set
        "tr": None,
        "center": np.float32([[1.5, -2.25, np.nan]]),
    }


def _check(arrays):
    words, offs = layout(arrays)
    assert words.dtype == np.int32 and words.ndim == 1
    present = [k for k, a in arrays.items() if a is not None and np.size(a)]
    assert sorted(offs) == sorted(present)                                  # absent and empty parts have no offset ...
    assert len(words) == sum(np.asarray(arrays[k]).nbytes // 4 for k in present)      # ... and no words: nothing but the parts, no padding
    spans = []
    for k in present:
        a = np.ascontiguousarray(arrays[k])
        n = a.nbytes // 4
        assert isinstance(offs[k], int) and 0 <= offs[k] <= len(words) - n
        assert words[offs[k]:offs[k] + n].tobytes() == a.tobytes(), k         # bit-exact, NaN payloads and top bits included
        assert (4 * offs[k]) % a.dtype.itemsize == 0, k                       # an 8-byte part starts at an even word
        spans.append((offs[k], offs[k] + n))
    spans.sort()
    assert all(a1 == b0 for (_, a1), (b0, _) in zip(spans, spans[1:]))      # the parts tile the buffer
    return offs


def test_ptr_is_the_int32_prefix_sum():
    p = ptr([3, 0, 5])
    assert p.dtype == np.int32 and p.tolist() == [0, 3, 3, 8]
    assert ptr([]).tolist() == [0] and ptr(np.asarray([2 ** 20] * 3, dtype=np.int64))[-1] == 3 * 2 ** 20


def test_layout_reads_back_and_aligns_every_part():
    arrays = _arrays()
    offs = _check(arrays)
    # the 8-byte parts come first in the mapping's order, then the 4-byte parts in the mapping's order
    assert sorted(offs, key=offs.get) == ["tor", "tables", "lig_ptr", "pos", "mask_bits", "center"]
    assert "tr" not in offs and "no_bonds" not in offs
    words, offs = layout({"tr": None, "no_bonds": np.zeros((0, 2), np.int32)})
    assert len(words) == 0 and words.dtype == np.int32 and offs == {}


def test_no_order_of_the_mapping_puts_an_8_byte_part_at_an_odd_word():
    arrays = _arrays()
    names = ["pos", "tor", "mask_bits", "tables", "tr", "no_bonds"]      # two odd-length 4-byte parts around two 8-byte parts
    for order in itertools.permutations(names):
        _check({k: arrays[k] for k in order})


def test_layout_refuses_items_it_cannot_align():
    for bad in (np.zeros(3, np.uint8), np.zeros(2, np.float16), np.zeros(2, np.complex128)):
        with pytest.raises(TypeError):
            layout({"ok": np.zeros(1, np.int32), "bad": bad})
