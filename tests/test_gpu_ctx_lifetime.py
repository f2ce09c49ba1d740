"""A context owns every buffer the library allocates on its behalf: destroying it gives the device memory back -- the scratch of
the entry points that keep some between calls (feature extraction, ring registration, the voxel filters, the tree build, the
hidden odometry node) included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def workload(synth):
    """Inputs of one `use` of a context, sized so that the entry points' scratch (a few hundred thousand points through the two
    filters and the ring registration) is most of what a used context holds: the map and its trees are small."""
    rng = np.random.default_rng(11)
    world = synth.World(half_extent=60.0, wall_half=55.0)
    corner, surf, _, sweep, ranges = synth.make_scan(world, 64, 2400, seed=5, full=True)  # 64 rings of <= 2400 points

    def cloud(n):  # {x, y, z, intensity} in a 100 m box, 8 m high
        return np.concatenate([rng.uniform(-50, 50, (n, 2)), rng.uniform(-2, 6, (n, 1)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    n_raw = 400000  # a raw driver cloud: elevations inside the ring table's [-15, 15] degrees
    az, el, r = rng.uniform(0, 2 * np.pi, n_raw), np.radians(rng.uniform(-14.5, 14.5, n_raw)), rng.uniform(2, 80, n_raw)
    raw = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), np.zeros(n_raw)], 1).astype(np.float32)
    return dict(sweep=sweep, ranges=ranges, corner=corner, surf=surf, raw=raw, big=cloud(400000), a=cloud(200000), b=cloud(200000))


def use(pkg, ctx, w):
    """Every entry point that keeps scratch in its context, once; returns the clouds they made (the same on every context)."""
    f = pkg.scan_registration.extract_features(ctx, w["sweep"], w["ranges"])
    reg, _ = pkg.scan_registration.multiscan_register(ctx, w["raw"], -15.0, 15.0, 16)
    g = pkg.voxel_grid(ctx, w["big"], 0.4)
    ga, gb = pkg.voxel_grid2(ctx, w["a"], w["b"], 0.4)
    ctx.map_set(w["corner"], w["surf"])  # both kd-trees: the corner tree on the context's second stream
    ctx.odometry_match(f["less_sharp"], f["less_flat"], f["sharp"], f["flat"], np.zeros(6, np.float32))  # the hidden node
    return [f["less_flat"], reg, g, ga, gb]


def test_destroyed_contexts_give_their_scratch_back(pkg, workload):
    """Eight contexts alive at the same time (so that their streams are distinct handles), each used, all closed: the device's
    free memory is back within what ONE used context holds.  (Not create / use / close in a loop: the runtime tends to hand a
    new stream the address of the one just destroyed, and scratch that is looked up by stream handle then seems to be
    released when it is only inherited.)  Eight and `lost < one` are conditions, not tuned numbers: scratch that stays behind
    shows as soon as it is more than an eighth of a used context.

    What the HIP runtime keeps has to be settled first, and one context does not do that: the runtime spreads streams over its
    hardware queues (four here) and gives each queue, for good, the private-memory area of the largest kernel it has run
    (odom_gn_kernel: 336 bytes per lane, 52 MiB per queue; the tree build's kd_build_big_kernel: 256).  One context reaches two
    queues, eight reach all: measured on the MI355X with a settling step of one context only, 382 MiB stayed behind after the
    eight -- and not one byte more after eight further ones.  So the measured round of eight is run once before anything is
    recorded; the four steps of the measurement follow as they stand.  Scratch that leaks per context is not forgiven by that:
    the measured round leaks it again."""
    import torch

    def free():
        return torch.cuda.mem_get_info()[0]

    def eight_alive(ref):
        ctxs = [pkg.Context(0) for _ in range(8)]
        for c in ctxs:
            got = use(pkg, c, workload)
            for x, y in zip(got, ref or got):
                assert x.shape == y.shape and np.array_equal(bits(x), bits(y))
        held = free()
        for c in ctxs:
            c.close()
        return got, held
    ref, _ = eight_alive(None)  # the runtime's per-queue state
    c = pkg.Context(0)  # (a) settles what the runtime and the library keep per process
    use(pkg, c, workload)
    c.close()
    free0 = free()
    c = pkg.Context(0)  # (b) what one used context holds
    use(pkg, c, workload)
    one = free0 - free()
    c.close()
    _, held = eight_alive(ref)  # (c)
    lost = free0 - free()  # (d)
    print("one used context %.1f MiB, eight %.1f MiB, lost after closing them %.1f MiB" % (one / 2 ** 20, (free0 - held) / 2 ** 20, lost / 2 ** 20))
    assert one > 64 << 20  # (the filters' scratch for 400 k points alone is tens of megabytes: a context that shows less inherited it)
    assert lost < one
