"""The reservation protocol of csrc/frame_device.h wg_fetch_pixels restated on integers: four consumers (the waves of a workgroup)
share one 64-bit word and change it only by compare-and-swap, or — the one that holds `fetching` — by a plain store.  Every memory
operation of a consumer is one step of a generator, so a scheduler can interleave the consumers any way it likes.

The word, low bit first (the device's packing):
    used 11 | valid 11 | fetching 1 | exhausted 1 | first tile 24 | frame 7 | shard 6
The work is a list of chunks per shard, each with an identity (frame, first tile) no other chunk has and a number of valid slots
(0 = padding); the shard's counter hands out chunk indices.  What the device does with a slot (slot -> pixel) is not modelled."""

FETCHING, EXHAUSTED = 1 << 22, 1 << 23
CAS_TRIES = 8


def pack(shard, frame, tile0, valid, exhausted=False):
    assert 0 <= shard < 64 and 0 <= frame < 128 and 0 <= tile0 < (1 << 24) and 0 <= valid < (1 << 11)
    return (shard << 55) | (frame << 48) | (tile0 << 24) | (EXHAUSTED if exhausted else 0) | (valid << 11)


def used(s):
    return s & 0x7ff


def valid(s):
    return (s >> 11) & 0x7ff


def ident(s):
    return (s >> 48) & 0x7f, (s >> 24) & 0xffffff


def shard_of(s):
    return (s >> 55) & 63


class Device:
    """What all workgroups share: the shards' counters (device memory) and the chunks behind them."""

    def __init__(self, chunks):
        self.chunks = chunks                       # chunks[shard] = [(frame, tile0, valid), ...]
        self.counter = [0] * len(chunks)
        self.adds = 0                              # device-scope atomics


class Workgroup:
    """The LDS word of one workgroup."""

    def __init__(self, dev, home):
        self.dev = dev
        self.word = pack(home, 0, 0, 0)
        self.installed = {self.word}               # every word a store ever wrote
        self.fetchers = 0                          # consumers between winning `fetching` and their install (must never exceed 1)

    def cas(self, expect, new):
        old = self.word
        if old == expect:
            self.word = new
        return old


def fetch_run(wg, shard):
    """wg_fetch_run: one add to the shard's counter, the dry-shard probe, the word to install.  Yields once per memory operation."""
    dev = wg.dev
    n = len(dev.chunks[shard])
    dev.adds += 1
    base = dev.counter[shard]
    dev.counter[shard] += 1
    yield
    nshard, exh = shard, False
    if base + 1 >= n:                              # this shard is (now) dry
        seen = list(dev.counter)                   # one load per lane
        yield
        avail = [q for q in range(len(seen)) if q != shard and seen[q] < len(dev.chunks[q])]
        if not avail:
            exh = True
        else:
            after = [q for q in avail if q > shard]
            nshard = (after or avail)[0]
    if base < n:
        frame, tile0, v = dev.chunks[shard][base]
        return pack(nshard, frame, tile0, v, exh) if v else pack(nshard, 0, 0, 0, exh)
    return pack(nshard, 0, 0, 0, exh)


def refill(wg, n, got, log):
    """wg_fetch_pixels for n dead lanes: appends the slots it took to `got` as ((frame, tile0), index) and every word it read to `log`.
    Returns (lanes served, saw exhausted)."""
    taken = 0
    for _ in range(2):
        tries = 0
        while True:
            if tries == CAS_TRIES:
                return taken, False
            tries += 1
            s = wg.word
            log.append(s)
            yield
            avail = valid(s) - used(s)
            if avail:
                k = min(n - taken, avail)
                fetch = k == avail and not s & EXHAUSTED
                s2 = (s + k) | (FETCHING if fetch else 0)
            elif s & EXHAUSTED:
                return taken, True
            elif s & FETCHING:
                return taken, False
            else:
                k, fetch, s2 = 0, True, s | FETCHING
            old = wg.cas(s, s2)
            if old == s and fetch:
                wg.fetchers += 1
                assert wg.fetchers == 1, "two consumers hold `fetching`"
            yield
            if old == s:
                break
        got.extend((ident(s), used(s) + j) for j in range(k))
        taken += k
        if not fetch:
            return taken, k == avail
        ns = yield from fetch_run(wg, shard_of(s))
        assert wg.word == s2, "the word changed under the consumer that holds `fetching`"
        wg.fetchers -= 1
        wg.word = ns
        wg.installed.add(ns)
        yield
        if taken == n:
            break
    return taken, False


def consumer(wg, rng, got, log, trips):
    """A wave: refills of random size until it sees `exhausted`; a bounded number of trips, like the device's scheduler loop."""
    for _ in range(trips):
        _, done = yield from refill(wg, rng.randint(1, 64), got, log)
        if done:
            return True
    return False


def run(chunks, homes, rng, consumers=4, trips=100000):
    """One workgroup per entry of `homes` (its home shard), `consumers` consumers each, interleaved at random until all have seen
    `exhausted`.  Returns (device, workgroups, slots per consumer, words read per workgroup)."""
    dev = Device(chunks)
    wgs = [Workgroup(dev, h) for h in homes]
    got = [[] for _ in range(consumers * len(wgs))]
    logs = [[] for _ in wgs]
    live = {i: consumer(wgs[i // consumers], rng, got[i], logs[i // consumers], trips) for i in range(len(got))}
    finished = {}
    while live:
        i = rng.choice(sorted(live))
        try:
            next(live[i])
        except StopIteration as e:
            finished[i] = e.value
            del live[i]
    assert all(finished.values()), "a consumer ran out of trips before the work was exhausted"
    return dev, wgs, got, logs
