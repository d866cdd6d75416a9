"""The creature order of a world stated on the host (include/rem2d_order.h), shared by tests/test_order_host.py (numpy alone) and
tests/test_order_gpu.py: what control_model.py is for observe / control and stream_model.py for the refill.

Plain numpy, and nothing of the package that computes an order is imported.  Four statements:

``device_order``   the order rem2d_rebalance_kernel writes, from the sentence in its header comment (csrc/rem2d_pipeline.h): a STABLE
                   counting sort of the world's creatures by cost class -- those that used every position iteration in the last
                   step first, then those that used three or more, then the rest, each class in its static order -- in both halves
                   of the array, the padding slots holding themselves.  Written as a counting sort (count, prefix, place); the
                   host test compares it with numpy's stable argsort.
``host_order``     what BatchedModular2D.rebalance() installs through rem2d_world_set_order: two classes.
``threads_for``    launch_rebalance's thread count (csrc/rem2d.hip).
``reorder_points`` at which queued-step counts a re-ordering launch runs, restated from the comments of tiles_launch_step and
                   tiles_launch_train (csrc/rem2d.hip).
"""
import numpy as np

WAVE = 64
MAX_THREADS = 1024
CHUNK = 256          # creatures a thread takes before the workgroup is doubled


def cost_class(positers, pos_iters, classes=3):
    """0 = used every position iteration, 1 = three or more (three classes only), last = the rest"""
    p = np.asarray(positers, dtype=np.int64)
    if classes == 2:
        return np.where(p >= pos_iters, 0, 1)
    if classes == 3:
        return np.where(p >= pos_iters, 0, np.where(p >= 3, 1, 2))
    raise ValueError("classes must be 2 or 3")


def counting_sort(cls, classes):
    """Stable: creature e of class k goes behind every creature of a class < k and behind the creatures < e of class k."""
    cls = np.asarray(cls)
    n = len(cls)
    count = [0] * classes
    for k in range(classes):
        count[k] = int((cls == k).sum())
    start, total = [], 0
    for k in range(classes):
        start.append(total)
        total += count[k]
    assert total == n, "a class outside 0 .. classes - 1"
    out = np.full(n, -1, dtype=np.int32)
    for k in range(classes):
        members = np.nonzero(cls == k)[0]              # ascending: the static order inside the class
        out[start[k]:start[k] + count[k]] = members
    return out


def device_order(positers, pos_iters, n_padded, classes=3):
    """int32 [2, n_padded]: the array after one launch of the re-ordering kernel on a world of len(positers) creatures"""
    n = len(positers)
    assert 0 < n <= n_padded
    half = np.arange(n_padded, dtype=np.int32)                           # padding slots keep themselves
    half[:n] = counting_sort(cost_class(positers, pos_iters, classes), classes)
    return np.stack([half, half])                                        # the second half equals the first


def host_order(positers, pos_iters):
    """int32 [n]: the creatures with positers >= pos_iters first, in their static order, the others behind in theirs"""
    return counting_sort(cost_class(positers, pos_iters, 2), 2)


def identity(n_padded):
    half = np.arange(n_padded, dtype=np.int32)
    return np.stack([half, half])


def is_valid(order, n, n_padded):
    """What every read is held to first: [2, n_padded], both halves equal, a permutation of the creatures, identity padding"""
    order = np.asarray(order)
    if order.shape != (2, n_padded) or not np.array_equal(order[0], order[1]):
        return False
    if not np.array_equal(order[0, n:], np.arange(n, n_padded)):
        return False
    head = order[0, :n].astype(np.int64)
    if head.min() < 0 or head.max() >= n:
        return False
    return bool((np.bincount(head, minlength=n) == 1).all())      # every creature in exactly one slot


def threads_for(n_envs):
    """64, doubled while below 1 024 and threads * 256 < n_envs"""
    threads = WAVE
    while threads < MAX_THREADS and threads * CHUNK < n_envs:
        threads *= 2
    return threads


def chunk(n_envs, threads=None):
    """creatures per thread: ceil(n / T); thread t takes [t * per, (t + 1) * per) cut at n"""
    threads = threads or threads_for(n_envs)
    return -(-n_envs // threads)


def train_segments(calls, every):
    """The step train's launches: every call cut into segments of at most `every` steps (every <= 0: one launch per call)"""
    out = []
    for n in calls:
        segs, left = [], n
        while left > 0:
            seg = min(left, every) if every > 0 else left
            segs.append(seg)
            left -= seg
        out.append(segs)
    return out


def reorder_points(calls, every, form, queued0=0):
    """[per call] the queued-step counts q in front of which a re-ordering launch runs -- it reads the state after q env-steps.

    form "step" (one launch sequence per env-step: tiles, velpost, with or without graph replay): in front of queued step q when
    q > 0 and q % every == 0.  form "train": in front of a segment (train_segments) when q > 0 and q - (q at the last re-ordering
    launch, 0 before the first) >= every.  `queued0`: the steps the world has queued before the first call -- counted from its
    creation; a reset does not rewind it."""
    if form not in ("step", "train"):
        raise ValueError(form)
    out, q, last = [], queued0, 0
    for n, segs in zip(calls, train_segments(calls, every)):
        pts = []
        if every > 0 and form == "step":
            for _ in range(n):
                if q > 0 and q % every == 0:
                    pts.append(q)
                q += 1
        elif every > 0:
            for seg in segs:
                if q > 0 and q - last >= every:
                    pts.append(q)
                    last = q
                q += seg
        else:
            q += n
        out.append(pts)
    return out
