"""`drin_workgroups_per_mention` (include/drin_hip.h): into how many workgroups the row-streaming kernels of the two inference paths
cut a mention's candidate list for a call size.  Host-only, no device: the answer over call sizes either side of both gates, every
list length 1 .. 1100, both paths and four width / activation classes against a restatement of the two rules
(`FusedLayout::build`, csrc/fused_forward.hip; `cached_chunk_candidates`, csrc/entity_cache.hip), and - from the restatement - the
two properties every kernel that re-derives `per = ceil(N / chunks)` relies on.  tests/test_gpu_chunk_bands.py asks this function
which cut each of its cases takes; this file pins what it answers."""
import pytest

from tests.helpers import workgroups_per_mention

BATCHES = (1, 1023, 1024, 2047, 2048, 4096)
# (D, R, vertex activation): tiny, guarded, exact, and the exact widths under an activation that has no exact cached-pairs form
WIDTHS = [(64, 128, "gelu"), (512, 1024, "gelu"), (768, 2048, "gelu"), (768, 2048, "silu")]


def _candidates_per_workgroup(B, cached, exact):
    """The two rules: the folded path by call size alone; the cached path 16 unless its exact instantiation runs."""
    if cached:
        return (128 if B >= 2048 else 64) if exact else 16
    return 128 if B >= 2048 else 48 if B >= 1024 else 16


@pytest.mark.parametrize("cached", [False, True], ids=["folded", "cached"])
@pytest.mark.parametrize("D,R,act", WIDTHS, ids=[f"{d}x{r}_{a}" for d, r, a in WIDTHS])
def test_workgroups_per_mention_over_call_sizes_and_list_lengths(D, R, act, cached):
    exact = (D, R, act) == (768, 2048, "gelu")
    seen = set()
    for B in BATCHES:
        S = _candidates_per_workgroup(B, cached, exact)
        seen.add(S)
        for N in range(1, 1101):
            got = workgroups_per_mention(D, R, B, N, cached, act, num_entities=23 if cached else 0)
            assert got == -(-N // S), (D, R, act, cached, B, N, got)
    assert seen == ({16} if cached and not exact else {64, 128} if cached else {16, 48, 128})


def test_exact_widths_under_a_generic_activation_fall_back_to_one_group_on_the_cached_side():
    """768 / 2048 with silu vertices: `k_cached_pairs<3, 8, false, true>` keeps ONE 16-candidate group per workgroup whatever the
    call size; the folded path's cut does not look at the widths."""
    for B in BATCHES:
        assert workgroups_per_mention(768, 2048, B, 65, True, "silu", num_entities=23) == 5
        assert workgroups_per_mention(768, 2048, B, 65, True, "gelu", num_entities=23) == (1 if B >= 2048 else 2)
        assert workgroups_per_mention(768, 2048, B, 65, False, "silu") == workgroups_per_mention(64, 128, B, 65, False, "gelu")


@pytest.mark.parametrize("S", [16, 48, 64, 128])
def test_rederived_chunk_length_fits_and_leaves_no_workgroup_empty(S):
    """The launchers pass `chunks = ceil(N / S)`; every kernel re-derives `per = ceil(N / chunks)` and workgroup c takes
    candidates [c per, min(N, (c + 1) per)).  `per <= S`: the LDS / register budget sized for S candidates holds.
    `(chunks - 1) per < N`: the last workgroup has at least one candidate - its partial is a sum, never uninitialised."""
    for N in range(1, 4101):
        chunks = -(-N // S)
        per = -(-N // chunks)
        assert per <= S, (N, S, chunks, per)
        assert (chunks - 1) * per < N, (N, S, chunks, per)
        assert chunks * per >= N
