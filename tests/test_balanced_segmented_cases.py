"""CPU-only checks of the numpy model of the balanced segmented sort (tests/balanced_segmented_cases.py): the clean model
equals np.lexsort((keys, segment id)) on every case tests/test_balanced_segmented_gpu.py runs, its split words follow the
rule's arithmetic, and every planted fault changes one of those cases -- the keys and values, or (fault 8) the split words.
At 32 compute units: the cases scale with the CU count and are the same cases at 256."""
import numpy as np
import pytest

import balanced_segmented_cases as model

CUS = 32


@pytest.fixture(scope="module")
def cases():
    return model.cases(CUS)


@pytest.fixture(scope="module")
def references(cases):
    return {name: model.reference(*case) for name, case in cases.items()}


def test_the_clean_model_is_the_stable_segmented_sort(cases, references):
    for name, (keys, values, offsets) in cases.items():
        got_k, got_v, _ = model.sort_model(keys, values, offsets, CUS)
        want_k, want_v = references[name]
        assert np.array_equal(got_k, want_k), name
        assert np.array_equal(got_v, want_v), name


def test_the_split_words_of_the_cases(cases):
    words = {name: model.split_words(case[2], CUS) for name, case in cases.items()}
    assert words["n65536"] == (1, 0, 0, 16384)
    assert words["n65537"] == (1, 1, 5, 16384)                 # four pieces of 16384 and one of one key
    assert words["k_quarter"][:2] == (CUS // 4, CUS // 4)
    assert words["k_half"][:3] == (CUS // 2, 0, 0)
    assert words["one_among"][:3] == (CUS + 1, 0, 0)
    assert words["one_among_spread"][:3] == (CUS + 1, 1, 16)
    listed, spread, pieces, length = words["two_tiles"]
    assert (listed, spread) == (1, 1) and length == 2 * 16384 + 256 and length > model.TILE and pieces == CUS
    assert all(words[f"neighbours{r}"][:2] == (4, 2) for r in range(4))
    assert words["passes"][:2] == (len(model.PASS_KINDS),) * 2
    for name, case in cases.items():   # the caps the host derives hold
        n = len(case[0])
        assert words[name][1] <= model.spread_cap(n, CUS) and words[name][2] <= model.piece_cap(n, CUS), name


def test_an_all_equal_spread_segment_touches_no_scratch(cases):
    keys, values, offsets = cases["passes"]
    _, _, touched = model.sort_model(keys, values, offsets, CUS)
    at = model.PASS_KINDS.index("equal")
    assert not touched[offsets[at]:offsets[at + 1]].any()
    assert touched[offsets[0]:offsets[1]].all()   # (a segment of uniform keys does)


@pytest.mark.parametrize("fault", model.FAULTS)
def test_every_fault_changes_a_case_the_gpu_file_runs(cases, references, fault):
    changed = []
    for name, (keys, values, offsets) in cases.items():
        if fault == 8:
            if model.split_words(offsets, CUS, fault) != model.split_words(offsets, CUS):
                changed.append(name)
            continue
        got_k, got_v, _ = model.sort_model(keys, values, offsets, CUS, fault)
        if not (np.array_equal(got_k, references[name][0]) and np.array_equal(got_v, references[name][1])):
            changed.append(name)
            break
    assert changed, f"fault {fault} changes no case"
