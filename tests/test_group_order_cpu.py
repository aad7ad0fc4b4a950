"""FileDataset.configure(group=K) without a GPU: the epoch order made of full groups of K same-size samples
(data_loaders/files.py) that dataset.DeviceFeed(samples_per_step=K) trains on, epoch_steps, and the untouched default order."""
import numpy as np
import pytest

SCALE = 96
# three size classes at scale 96: (96, 128), (128, 96) and (96, 96)
SIZES = [(375, 500), (500, 375), (500, 500)]


def _dataset(counts, seed=0):
    """A FileDataset over sum(counts) records, counts[c] of them of SIZES[c], in a shuffled annotation order."""
    from data_loaders.files import FileDataset
    sizes = [SIZES[c] for c, n in enumerate(counts) for _ in range(n)]
    sizes = [sizes[i] for i in np.random.default_rng(seed).permutation(len(sizes))]

    class Fake(FileDataset):
        def __init__(self):
            super(Fake, self).__init__()
            self._class_names = ['a', 'b']
            self._keep({'image_file': 'img%d.jpg' % i, 'boxes': np.array([[1, 2, 3, 4]], np.float32),
                        'class_ids': np.zeros(1, np.int32), 'image_size': hw} for i, hw in enumerate(sizes))
    return Fake()


def _greedy(keys, k):
    """The groups the feed forms: the next sample plus those that follow it while they have its key, k at most."""
    groups = []
    for i, key in enumerate(keys):
        if groups and len(groups[-1]) < k and keys[groups[-1][0]] == key:
            groups[-1].append(i)
        else:
            groups.append([i])
    return groups


def test_the_three_sizes_are_three_network_input_sizes():
    import dataset
    assert len({dataset.rescale_size(hw, SCALE) for hw in SIZES}) == 3


@pytest.mark.parametrize('world', [1, 2])
def test_group_order_is_a_permutation_of_full_groups_with_partial_ones_only_at_the_end(world):
    import dataset
    from data_loaders import files
    k = 3
    counts = (700, 400, 301)                                  # none a multiple of 3; 1401 records
    assert all(n % k for n in counts) and sum(counts) // world > files.WINDOW      # more than one window on every rank
    seen = []
    for rank in range(world):
        dl = _dataset(counts).configure(seed=3, rank=rank, world=world, scale=SCALE, group=k)
        order = dl.epoch_order(0)
        plain = _dataset(counts).configure(seed=3, rank=rank, world=world).epoch_order(0)
        assert sorted(order) == sorted(plain) and len(set(order)) == len(order)       # this rank's shard, every index once
        assert order != plain
        keys = [dataset.rescale_size(dl.records[i]['image_size'], SCALE) for i in order]
        groups = _greedy(keys, k)
        partial = [g for g in groups if len(g) < k]
        # full groups first, then at most one partial group per size class, nothing after them
        assert len(partial) <= 3 and len({keys[g[0]] for g in partial}) == len(partial)
        assert groups[len(groups) - len(partial):] == partial
        per_class = {}
        for key in keys:
            per_class[key] = per_class.get(key, 0) + 1
        assert len(groups) == sum(-(-n // k) for n in per_class.values())             # as few steps as the sizes allow
        assert len(partial) == sum(1 for n in per_class.values() if n % k)
        assert dl.epoch_steps(0) == len(groups)
        # any rank's count from any rank, without iterating
        other = _dataset(counts).configure(seed=3, rank=(rank + 1) % world, world=world, scale=SCALE, group=k)
        assert other.epoch_steps(0, rank) == len(groups)
        # deterministic: a pure function of (seed, epoch, rank, world, scale, K)
        again = _dataset(counts).configure(seed=3, rank=rank, world=world, scale=SCALE, group=k)
        assert again.epoch_order(0) == order
        assert again.epoch_order(1) != order
        assert _dataset(counts).configure(seed=4, rank=rank, world=world, scale=SCALE, group=k).epoch_order(0) != order
        seen.append(set(order))
    if world == 2:
        assert not (seen[0] & seen[1]) and len(seen[0] | seen[1]) == sum(counts)      # ranks are disjoint and cover the records


def test_leftovers_are_carried_into_the_next_window_and_taken_first():
    import dataset
    from data_loaders import files
    k = 3
    dl = _dataset((700, 400, 301)).configure(seed=3, scale=SCALE, group=k)
    order = dl.epoch_order(0)
    plain = _dataset((700, 400, 301)).configure(seed=3).epoch_order(0)
    position = {i: p for p, i in enumerate(plain)}
    keys = [dataset.rescale_size(dl.records[i]['image_size'], SCALE) for i in order]
    mixed = 0
    for g in _greedy(keys, k):
        windows = [position[order[p]] // files.WINDOW for p in g]
        assert windows == sorted(windows)                     # inside a group the carried (earlier-window) samples come first
        mixed += len(set(windows)) > 1
    assert mixed > 0                                          # groups do span windows: leftovers were carried, not emitted


def test_group_wins_over_shape_runs_and_the_stream_follows_the_order():
    a = _dataset((40, 23, 12)).configure(seed=1, scale=SCALE, group=4, shape_runs=8, repeat=True)
    b = _dataset((40, 23, 12)).configure(seed=1, scale=SCALE, group=4, repeat=True)
    assert a.epoch_order(0) == b.epoch_order(0)
    it = iter(a)
    got = [next(it)['image_file'] for _ in range(75 + 5)]
    want = [a.records[i]['image_file'] for i in a.epoch_order(0) + a.epoch_order(1)[:5]]
    assert got == want
    assert a.epoch_steps(0) == 10 + 6 + 3


def test_group_zero_is_the_order_of_a_loader_that_never_heard_of_groups():
    """group=0 (and the argument left out) against the current order, written out: the (seed, epoch) permutation, the rank's
    stride, windows of WINDOW samples, shape_run_order per window with the seed (seed, epoch, rank, window)."""
    import dataset
    from data_loaders import files
    counts, seed, epoch, world, rank, runs = (500, 420, 333), 7, 2, 2, 1, 8
    for kw in ({'group': 0}, {}):
        dl = _dataset(counts).configure(seed=seed, rank=rank, world=world, scale=SCALE, shape_runs=runs, **kw)
        perm = np.random.default_rng([seed, epoch]).permutation(sum(counts))
        mine = [int(i) for i in perm[rank::world]]
        want = []
        for w0 in range(0, len(mine), files.WINDOW):
            win = mine[w0:w0 + files.WINDOW]
            keys = [dataset.rescale_size(dl.records[i]['image_size'], SCALE) for i in win]
            for chunk in files.shape_run_order(keys, runs, [seed, epoch, rank, w0 // files.WINDOW]):
                want.extend(win[j] for j in chunk)
        assert dl.epoch_order(epoch) == want
        assert dl.epoch_steps(epoch) == len(mine) == dl.epoch_length()
        plain = _dataset(counts).configure(seed=seed, rank=rank, world=world, **kw)
        assert plain.epoch_order(epoch) == mine


def test_parser_and_main_check_samples_per_step_before_touching_the_gpu():
    import train
    a = train.build_parser().parse_args(['--dataset', 'pascal', '/d/VOC2012', 'trainval', '--samples-per-step', '4'])
    assert a.samples_per_step == 4
    assert train.build_parser().parse_args([]).samples_per_step == 1
    for argv in (['--samples-per-step', '2'],                                                   # shapes: not a file dataset
                 ['--dataset', 'pascal', '/d/VOC2012', 'trainval', '--samples-per-step', '0'],
                 ['--dataset', 'pascal', '/d/VOC2012', 'trainval', '--samples-per-step', '17']):
        with pytest.raises(SystemExit):
            train.main(argv)


def test_feed_refuses_groups_without_ragged_mode_before_touching_the_device():
    import dataset

    class Loader(object):
        num_classes = 3

        def __iter__(self):
            raise AssertionError("the loader must not be read")

    with pytest.raises(ValueError, match='ragged'):
        dataset.DeviceFeed(Loader(), None, samples_per_step=2)
    for k in (0, 17):
        with pytest.raises(ValueError, match='samples_per_step'):
            dataset.DeviceFeed(Loader(), None, ragged=True, samples_per_step=k)
