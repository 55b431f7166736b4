"""The raw words behind torch.randint on the CPU generator (u2pl_amd.rng_words): the device-side contrastive sampling
applies the bounds to words the host read ahead, so `word % high` has to BE torch.randint, draw for draw, and reading
ahead must not move the generator."""
import numpy as np
import pytest
import torch

from u2pl_amd import rng_words as RW

SEEDS = [0, 5, 2 ** 31]
BOUNDS = [1, 2, 3, 255, 256, 12345, 50000, 2 ** 16 + 1, 2 ** 28 - 1, 2 ** 28, 2 ** 31 - 1]
SIZES = [1, 255, 256, 12800, 13056]


@pytest.mark.parametrize("seed", SEEDS)
def test_words_modulo_bound_are_randint(seed):
    for high in BOUNDS:
        for n in SIZES:
            torch.manual_seed(seed)
            torch.randint(7, (3,))                      # (not at the start of a block of 624)
            per = RW.words_per_draw(high)
            words = RW.peek_words(per * n)
            assert words.dtype == np.uint32 and words.shape == (per * n,)
            # below 2**28 -- every bound the device path admits -- a draw is words[k] % high; torch reduces a 64-bit value
            # of two words from there on (2**31 - 1 in this table), which randint_from_words restates and the device path
            # refuses (loss_helper keeps such a configuration on the host path)
            assert per == (1 if high < 2 ** 28 else 2)
            got = RW.randint_from_words(words, high, n)
            if per == 1:
                assert np.array_equal(got, (words.astype(np.uint64) % np.uint64(high)).astype(np.int64))
            ref = torch.randint(high, (n,)).numpy()
            assert np.array_equal(got, ref), (seed, high, n)


@pytest.mark.parametrize("seed", SEEDS)
def test_one_call_of_n_draws_is_n_calls_of_one_draw(seed):
    torch.manual_seed(seed)
    a = torch.randint(12345, (700,)).numpy()
    torch.manual_seed(seed)
    b = np.array([int(torch.randint(12345, (1,))) for _ in range(700)])
    assert np.array_equal(a, b)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("w,n", [(13056, 0), (13056, 1), (13056, 623), (13056, 624), (13056, 625), (13056, 13056), (248064, 13056 * 7)])
def test_peek_then_advance_equals_real_draws(seed, w, n):
    torch.manual_seed(seed)
    torch.randint(9, (11,))
    words = RW.peek_words(w)
    RW.advance(n)
    after_peek = torch.randint(2 ** 31 - 1, (64,)).numpy()
    state_peek = torch.get_rng_state()
    torch.manual_seed(seed)
    torch.randint(9, (11,))
    if n:
        real = torch.randint(50000, (n,)).numpy()
        assert np.array_equal(real, (words[:n].astype(np.uint64) % np.uint64(50000)).astype(np.int64))
    after_real = torch.randint(2 ** 31 - 1, (64,)).numpy()
    assert np.array_equal(after_peek, after_real)
    assert torch.equal(state_peek, torch.get_rng_state())


@pytest.mark.parametrize("seed", SEEDS)
def test_a_peek_leaves_the_generator_untouched(seed):
    torch.manual_seed(seed)
    for pre in (0, 1, 623, 624, 1000):
        if pre:
            torch.randint(3, (pre,))
        s0 = torch.get_rng_state().clone()
        RW.peek_words(2000)
        assert torch.equal(s0, torch.get_rng_state())
    g = torch.Generator().manual_seed(seed)
    s0 = g.get_state().clone()
    w = RW.peek_words(100, g)
    assert torch.equal(s0, g.get_state())
    assert np.array_equal(w.astype(np.int64) % 977, torch.randint(977, (100,), generator=g).numpy())
