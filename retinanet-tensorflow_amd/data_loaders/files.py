"""Epoch order, rank sharding and resume for the annotation-file readers (Pascal, COCO).

A reader parses its annotations once into a list of records -- {'image_file', 'boxes' [O,4] pixel corners (y1, x1, y2, x2),
'class_ids' [O], 'image_size' (h, w) from the annotation} -- and `FileDataset` turns that list into a sample stream:

  * unconfigured (the default), iteration yields the records once, in annotation order: the reference reader's own order
    (data_loaders/pascal.py, coco.py);
  * `configure(seed=...)`: epoch e is a full permutation of the records seeded by (seed, e) -- this replaces the reference's
    `ds.shuffle(4096)` buffer, a deliberate deviation: every epoch sees every record exactly once and the order is a pure
    function of (seed, epoch), so resuming is index arithmetic (`skip`);
  * sample i of an epoch's permutation goes to rank i % world;
  * shape_runs=K (with scale): the rank's sequence is cut into windows of WINDOW samples, each window is sorted by network
    input size (dataset.rescale_size of the annotated size -- nothing is decoded), cut into chunks of <= K same-size samples,
    and the chunk order is shuffled with a seed.  Consecutive steps then mostly share one input shape, so a graph-captured
    step replays instead of re-capturing; every sample still appears once per epoch.  K = 0: the plain permutation.
  * group=K (with scale; for dataset.DeviceFeed(samples_per_step=K), which trains on up to K consecutive samples of one
    network input size per step): the rank's sequence is cut into the same windows, and every window emits FULL groups of K
    same-size samples, in an order shuffled with the window's seed.  What is left of a size class -- fewer than K samples --
    is carried into the next window's pool, where it is taken first; only the end of the epoch emits partial groups, at most
    one per size class.  Every sample still appears once per epoch.  With group > 0 the order is the grouped one whatever
    shape_runs says (group wins): runs of one shape are then runs of groups only by chance, so a graph set is re-used through
    the trainer's cache rather than by adjacency.  `epoch_steps` counts the steps the feed makes of an epoch.

The stream position (`drawn`) is advanced by iteration and by `skip(n)`; an iterator starts where the position is.  With
repeat=True the stream runs on across epochs without end (training); otherwise it stops at the end of the current epoch.
"""
import numpy as np

from data_loaders.base import Base

WINDOW = 512


def shape_run_order(keys, k, seed):
    """Indices 0..len(keys)-1 reordered into chunks of <= k equal keys (sorted by key, stable), chunk order shuffled by `seed`.
    Returns the list of chunks (each a list of indices)."""
    order = sorted(range(len(keys)), key=lambda i: (keys[i], i))
    chunks, cur = [], []
    for i in order:
        if cur and (keys[cur[-1]] != keys[i] or len(cur) == k):
            chunks.append(cur)
            cur = []
        cur.append(i)
    if cur:
        chunks.append(cur)
    perm = np.random.default_rng(seed).permutation(len(chunks))
    return [chunks[j] for j in perm]


def greedy_groups(keys, k):
    """Sizes of the groups dataset.DeviceFeed(samples_per_step=k) forms from a stream with these size keys: the next sample
    plus those that follow it while they have its key, k at most."""
    sizes, i, n = [], 0, len(keys)
    while i < n:
        j = i + 1
        while j < n and j - i < k and keys[j] == keys[i]:
            j += 1
        sizes.append(j - i)
        i = j
    return sizes


class FileDataset(Base):
    """Base of the annotation-file readers: subclasses fill `self._records` and `self._class_names`."""

    def __init__(self):
        self._records = []
        self.skipped = 0                      # records dropped by a validating wrapper (data_loaders/inferred.py)
        self.drawn = 0
        self._epoch_cache = {}
        self.configure()

    @property
    def class_names(self):
        return self._class_names

    @property
    def records(self):
        return self._records

    def __len__(self):
        return len(self._records)

    def configure(self, seed=None, rank=0, world=1, shape_runs=0, scale=None, repeat=False, group=0):
        """Set the epoch order (see the module docstring); resets the cached orders, not the stream position.  group > 0 decides
        the order alone: shape_runs is then not applied."""
        assert 0 <= rank < world
        assert shape_runs == 0 or scale is not None, "shape runs group by network input size: they need the scale"
        assert group == 0 or scale is not None, "groups are formed by network input size: they need the scale"
        assert group >= 0
        self.seed, self.rank, self.world = seed, int(rank), int(world)
        self.shape_runs, self.scale, self.repeat = int(shape_runs), scale, bool(repeat)
        self.group = int(group)
        self._epoch_cache = {}
        return self

    def _keep(self, records):
        """Replace the record list (a validating wrapper drops records before any order is computed)."""
        self._records = list(records)
        self._epoch_cache = {}

    def epoch_length(self):
        """Samples of one epoch on this rank."""
        return len(range(self.rank, len(self._records), self.world))

    def max_objects(self):
        return max([len(r['class_ids']) for r in self._records] or [0])

    def max_image_pixels(self):
        return max([int(r['image_size'][0]) * int(r['image_size'][1]) for r in self._records] or [0])

    def _size_key(self, index):
        import dataset
        return dataset.rescale_size(self._records[index]['image_size'], self.scale)

    def _group_order(self, epoch, rank):
        """epoch_order with group > 0, of any rank, uncached: a pure function of (seed, epoch, rank, world, scale, group)."""
        n = len(self._records)
        if self.seed is None:
            perm = np.arange(n)
        else:
            perm = np.random.default_rng([int(self.seed), int(epoch)]).permutation(n)
        mine = [int(i) for i in perm[rank::self.world]]
        out, carried = [], {}                     # size key -> indices left over from earlier windows (fewer than `group`)
        for w0 in range(0, len(mine), WINDOW):
            pool = {}
            for i in mine[w0:w0 + WINDOW]:
                pool.setdefault(self._size_key(i), []).append(i)
            groups = []
            for key in sorted(set(pool) | set(carried)):
                members = carried.pop(key, []) + pool.get(key, [])            # carried samples are taken first
                full = len(members) // self.group * self.group
                groups += [members[g:g + self.group] for g in range(0, full, self.group)]
                if full < len(members):
                    carried[key] = members[full:]
            seed = [int(self.seed or 0), int(epoch), rank, w0 // WINDOW]
            for j in np.random.default_rng(seed).permutation(len(groups)):
                out.extend(groups[j])
        for key in sorted(carried):               # the end of the epoch: at most one partial group per size class
            out.extend(carried[key])
        return out

    def epoch_steps(self, epoch, rank=None):
        """Steps dataset.DeviceFeed(samples_per_step=group) makes of epoch `epoch` on `rank` (default: this rank): the number of
        groups it forms greedily from that rank's epoch order (one per sample with group <= 1).  Index arithmetic on the
        annotated sizes: nothing is read or decoded, and every rank can compute it for every other."""
        rank = self.rank if rank is None else int(rank)
        assert 0 <= rank < self.world
        if self.group <= 1:
            return len(range(rank, len(self._records), self.world))
        order = self.epoch_order(epoch) if rank == self.rank else self._group_order(epoch, rank)
        return len(greedy_groups([self._size_key(i) for i in order], self.group))

    def epoch_order(self, epoch):
        """Record indices of epoch `epoch` on this rank, in stream order."""
        got = self._epoch_cache.get(epoch)
        if got is not None:
            return got
        if self.group > 0:
            mine = self._group_order(epoch, self.rank)
            self._epoch_cache = {epoch: mine}
            return mine
        n = len(self._records)
        if self.seed is None:
            perm = np.arange(n)
        else:
            perm = np.random.default_rng([int(self.seed), int(epoch)]).permutation(n)
        mine = [int(i) for i in perm[self.rank::self.world]]
        if self.shape_runs > 0:
            import dataset
            out = []
            for w0 in range(0, len(mine), WINDOW):
                win = mine[w0:w0 + WINDOW]
                keys = [dataset.rescale_size(self._records[i]['image_size'], self.scale) for i in win]
                seed = [int(self.seed or 0), int(epoch), self.rank, w0 // WINDOW]
                for chunk in shape_run_order(keys, self.shape_runs, seed):
                    out.extend(win[j] for j in chunk)
            mine = out
        self._epoch_cache = {epoch: mine}     # one epoch at a time: a COCO epoch is ~10^5 indices
        return mine

    def skip(self, n):
        """Advance the stream by n samples (resume: the checkpoint stores how many were drawn)."""
        self.drawn += int(n)

    def sample(self, index):
        r = self._records[index]
        return {'image_file': r['image_file'], 'boxes': np.array(r['boxes'], np.float32).reshape(-1, 4),
                'class_ids': np.array(r['class_ids'], np.int32).reshape(-1), 'image_size': tuple(r['image_size'])}

    def __iter__(self):
        length = self.epoch_length()
        if length == 0:
            return
        first_epoch = self.drawn // length
        while True:
            epoch, pos = divmod(self.drawn, length)
            if epoch != first_epoch and not self.repeat:
                return
            order = self.epoch_order(epoch)
            self.drawn += 1
            yield self.sample(order[pos])
