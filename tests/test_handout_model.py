"""Off the GPU: the reservation protocol of the per-workgroup tile hand-out (csrc/frame_device.h wg_fetch_pixels, restated in
tests/handout_model.py) under random interleavings of four consumers per workgroup, refills of 1..64 lanes, chunks of 0..511 slots:
every slot is handed out exactly once, no consumer ever reads a word that was not installed whole or derived from one by a
compare-and-swap, one consumer at a time holds `fetching`, and the device-scope atomics number one per chunk and dry-shard visit."""
import random

import pytest

import handout_model as hm


def random_work(rng, n_shards, max_chunks):
    """chunks[shard] = [(frame, first tile, valid slots)]: identities unique over the whole launch, a third of the chunks padding or ragged"""
    chunks, tile = [], 0
    for _ in range(n_shards):
        row = []
        for _ in range(rng.randint(0, max_chunks)):
            v = rng.choice([0, rng.randint(1, 511), rng.randint(1, 7) * 64])
            row.append((rng.randint(0, 63), tile, v))
            tile += 8
        chunks.append(row)
    return chunks


@pytest.mark.parametrize("seed", range(40))
def test_every_slot_exactly_once(seed):
    rng = random.Random(0xA11 + seed)
    n_shards = rng.choice([1, 2, 4, 8])
    chunks = random_work(rng, n_shards, rng.choice([0, 1, 3, 12]))
    homes = [rng.randrange(n_shards) for _ in range(rng.choice([1, 1, 2, 5]))]
    dev, wgs, got, logs = hm.run(chunks, homes, rng)
    want = sorted(((f, t), j) for row in chunks for f, t, v in row for j in range(v))
    have = sorted(s for g in got for s in g)
    assert have == want, (len(have), len(want))
    # every word a consumer read: an installed word, possibly advanced by compare-and-swaps (more used, `fetching` at the drain)
    for wg, log in zip(wgs, logs):
        by_ident = {}
        for w in wg.installed:
            by_ident.setdefault((hm.ident(w), hm.valid(w), hm.shard_of(w), bool(w & hm.EXHAUSTED)), w)
        for s in log:
            assert (hm.ident(s), hm.valid(s), hm.shard_of(s), bool(s & hm.EXHAUSTED)) in by_ident, hex(s)
            assert hm.used(s) <= hm.valid(s), hex(s)
            if s & hm.FETCHING:
                assert hm.used(s) == hm.valid(s) and not s & hm.EXHAUSTED, hex(s)     # set only at a drain, never on the last chunk
        assert wg.fetchers == 0 and wg.word & hm.EXHAUSTED and hm.used(wg.word) == hm.valid(wg.word)
    # one add per chunk, and at most one more per workgroup and shard it found dry
    n_chunks = sum(len(row) for row in chunks)
    assert n_chunks <= dev.adds <= n_chunks + len(homes) * (n_shards + 1), (dev.adds, n_chunks)


def test_a_consumer_alone_and_an_empty_launch():
    rng = random.Random(7)
    dev, wgs, got, _ = hm.run([[]], [0], rng, consumers=1)
    assert got == [[]] and dev.adds == 1
    dev, wgs, got, _ = hm.run([[(3, 40, 100)]], [0], rng, consumers=1)
    assert sorted(got[0]) == [((3, 40), j) for j in range(100)] and dev.adds == 1
