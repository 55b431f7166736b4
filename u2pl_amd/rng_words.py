"""Raw 32-bit words of torch's CPU generator, ahead of the draws that will consume them.

`torch.randint(high, (n,))` on the CPU generator (high < 2**28) is `word % high` over n consecutive raw mt19937 words
(tests/test_sampling_words_cpu.py holds it to that).  The word stream does not depend on `high`, so the words of draws
whose bounds are not known yet can be read now and the bounds applied later -- on the device, for the contrastive
sampling (loss_helper.py:179-196 of the reference draws them on the host).

peek_words() reads the generator's state bytes, runs numpy's MT19937 (the same recurrence and tempering) from them and
leaves the generator untouched; advance() consumes words the way the draws would have."""
import numpy as np
import torch

# CPUGeneratorImpl's serialised state: {uint64 seed; int32 left; int32 seeded; uint64 next; uint64 state[624]; ...normal-sample cache}
_OFF_LEFT, _OFF_NEXT, _OFF_KEY, _N = 8, 16, 24, 624


def _mt_from_state(state_bytes):
    raw = state_bytes.numpy()
    if raw.dtype != np.uint8 or raw.size < _OFF_KEY + 8 * _N:
        raise RuntimeError("rng_words: unexpected CPU generator state (%d bytes)" % raw.size)
    left = int(raw[_OFF_LEFT:_OFF_LEFT + 4].view(np.int32)[0])
    nxt = int(raw[_OFF_NEXT:_OFF_NEXT + 8].view(np.uint64)[0])
    key = raw[_OFF_KEY:_OFF_KEY + 8 * _N].view(np.uint64)
    if not (1 <= left <= _N and 0 <= nxt <= _N) or int(key.max()) >> 32:
        raise RuntimeError("rng_words: unexpected CPU generator state (left %d, next %d)" % (left, nxt))
    # at::mt19937 regenerates its block when --left reaches 0 and then reads state[next++]; numpy regenerates at pos == 624
    pos = _N if left == 1 else nxt
    if left != 1 and left != _N - nxt + 1:
        raise RuntimeError("rng_words: inconsistent CPU generator state (left %d, next %d)" % (left, nxt))
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": key.astype(np.uint32), "pos": pos}}
    return bg


def peek_words(n, generator=None):
    """the next n raw 32-bit words of `generator` (default: the global CPU generator) as uint32 [n]; its state is not changed"""
    st = torch.get_rng_state() if generator is None else generator.get_state()
    return _mt_from_state(st).random_raw(int(n)).astype(np.uint32)


# torch draws a bound below 2**28 from ONE word (word % high); from 2**28 on it takes two words per draw and reduces the
# 64-bit value (first word high).  The device-side sampling implements the one-word rule only: its callers hold every
# bound (list capacity, ring capacity) below this.
ONE_WORD_BOUND = 1 << 28


def words_per_draw(high):
    return 1 if int(high) < ONE_WORD_BOUND else 2


def randint_from_words(words, high, n):
    """what torch.randint(high, (n,)) returns when the generator's next words are `words`: int64 [n] from the first
    n * words_per_draw(high) of them"""
    w = np.asarray(words, dtype=np.uint64)
    if words_per_draw(high) == 1:
        return (w[:n] % np.uint64(high)).astype(np.int64)
    return (((w[0:2 * n:2] << np.uint64(32)) | w[1:2 * n:2]) % np.uint64(high)).astype(np.int64)


def advance(n, generator=None):
    """consume n words, as n one-word draws of torch.randint would"""
    if n > 0:
        torch.randint(1, (int(n),), generator=generator)
