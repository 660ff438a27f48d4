"""Direction augmentation through its three doors: PackedLatentLoader(augment=dict(directions=...)), the
reference's augment_latents_with_directions (one file per variant) and fervit.data.augment_shard. Every latent
is compared bit for bit with `x + step * direction` in torch on the CPU; the loader's per-sample choices are
rebuilt by the host replica of the draw (latent_dirs_ref.dir_draw) from the loader's own batch seed."""
import os

import numpy as np
import pytest
import torch

import dropmask
import latent_dirs_ref as R
from elemwise import assert_bits_equal
from fervit import ops
from fervit._lib import check, lib
from fervit.data import PackedLatentDataset, PackedLatentLoader, augment_shard, write_shard

pytestmark = pytest.mark.gpu

N, B, SEED = 40, 16, 3
STEPS = (-2.0, -1.0, 1.0, 2.0)


def batch_seed(seed, epoch, k, rank=0):
    """PackedLatentLoader._augment's seed of batch k."""
    return (seed * 0x9E3779B97F4A7C15 + (epoch << 32) + k * 0xBF58476D1CE4E5B9 + rank) % (1 << 64)


@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    rng = np.random.default_rng(11)
    L, D = 18, 512
    lat = rng.standard_normal((N, L, D), dtype=np.float32)
    lab = rng.integers(0, 7, N)
    path = str(tmp_path_factory.mktemp("dir_aug") / "s.fwps")
    write_shard(path, lat, lab, [f"img/{i:03d}.png" for i in range(N)])
    return path, torch.from_numpy(lat), lab


def batches(epoch):
    perm = np.random.default_rng(SEED + epoch).permutation(N)
    return [perm[k * B:(k + 1) * B] for k in range(-(-N // B))]


@pytest.mark.parametrize("per_layer", [False, True])
def test_loader_shift_equals_the_replica(shard, per_layer):
    path, lat, lab = shard
    g = torch.Generator().manual_seed(5)
    K = 4
    dirs = torch.randn(*((K, 18, 512) if per_layer else (K, 512)), generator=g)
    steps = torch.tensor(STEPS)
    ds = PackedLatentDataset(path)
    ld = PackedLatentLoader(ds, batch_size=B, shuffle=True, seed=SEED, device="cuda",
                            augment=dict(directions=dirs.numpy() if per_layer else dirs))
    seen = set()
    for epoch in range(2):
        for k, ((x, y), idx) in enumerate(zip(ld, batches(epoch))):
            c = R.dir_draw(batch_seed(SEED, epoch, k), len(idx), K * len(STEPS), 1.0 / (1 + K * len(STEPS)))
            seen.update(c.tolist())
            assert_bits_equal(f"epoch {epoch} batch {k}", x.cpu(), R.shift_rows(lat[idx], dirs, steps, range(len(idx)), c))
            assert torch.equal(y.cpu(), torch.from_numpy(lab[idx]).long())
    assert len(seen) > 8 and min(seen) >= -1  # many different pairs were drawn
    ds.close()


def test_loader_dir_keep_and_steps_options(shard):
    """dir_keep = 1 leaves every sample as it is; dir_keep = 0 with one direction and one step shifts every
    sample by that pair."""
    path, lat, _ = shard
    d = torch.randn(1, 512, generator=torch.Generator().manual_seed(6))
    ds = PackedLatentDataset(path)
    for keep in (1.0, 0.0):
        ld = PackedLatentLoader(ds, batch_size=B, shuffle=False, seed=SEED, device="cuda",
                                augment=dict(directions=d, dir_steps=(0.5,), dir_keep=keep))
        got = torch.cat([x.cpu() for x, _ in ld])
        assert_bits_equal(f"dir_keep {keep}", got, lat if keep == 1.0 else lat + torch.tensor(0.5) * d[0][None, None])
    with pytest.raises(ValueError):
        PackedLatentLoader(ds, batch_size=B, device="cuda", augment=dict(directions=torch.zeros(2, 7)))
    with pytest.raises(ValueError):
        PackedLatentLoader(ds, batch_size=B, device=None, augment=dict(directions=d))
    ds.close()


def test_loader_without_directions_is_unchanged(shard):
    """Two epochs of a loader with the three LatentAugment stages and no `directions` key against the loader's
    calls before the direction stage existed: the batch gathered on the host, fer_latent_augment with the batch
    seed formula, nothing else."""
    path, lat, _ = shard
    ds = PackedLatentDataset(path)
    ld = PackedLatentLoader(ds, batch_size=B, shuffle=True, seed=SEED, device="cuda",
                            augment=dict(noise_std=0.05, scale_range=(0.9, 1.1), mask_prob=0.1))
    assert ld._dirs is None
    for epoch in range(2):
        for k, ((x, _), idx) in enumerate(zip(ld, batches(epoch))):
            ref = lat[idx].cuda()
            check(lib().fer_latent_augment(ref.data_ptr(), len(idx), 18 * 512, 0.05, 0.9, 1.1, 0.1,
                                           batch_seed(SEED, epoch, k), ops.stream()), "latent_augment")
            assert_bits_equal(f"epoch {epoch} batch {k}", x, ref)
            assert not torch.equal(x.cpu(), lat[idx])
    ds.close()


def test_loader_shift_then_augment(shard):
    """Both stages. Mask alone after the shift: the host replica of the mask draw, exact (dropped elements are
    +0.0, survivors keep the shifted bits). All three stages after the shift: fer_latent_augment applied to the
    replica's shifted batch under the same seed, bit for bit (the stages' own arithmetic is
    tests/test_gpu_edge_kernels.py's subject)."""
    path, lat, _ = shard
    K = 3
    dirs = torch.randn(K, 512, generator=torch.Generator().manual_seed(7))
    steps = torch.tensor(STEPS)
    ds = PackedLatentDataset(path)
    for aug in (dict(mask_prob=0.25), dict(noise_std=0.05, scale_range=(0.9, 1.1), mask_prob=0.1)):
        ld = PackedLatentLoader(ds, batch_size=B, shuffle=True, seed=SEED, device="cuda",
                                augment=dict(directions=dirs, dir_keep=0.2, **aug))
        for k, ((x, _), idx) in enumerate(zip(ld, batches(0))):
            seed = batch_seed(SEED, 0, k)
            nb = len(idx)
            c = R.dir_draw(seed, nb, K * len(STEPS), 0.2)
            shifted = R.shift_rows(lat[idx], dirs, steps, range(nb), c)
            if len(aug) == 1:
                um = dropmask.u01(dropmask.fer_hash(dropmask.sub_seeds(seed)[2], np.arange(nb * 18 * 512, dtype=np.uint64)))
                keep = torch.from_numpy(um > np.float32(0.25)).reshape(nb, 18, 512)
                want = torch.where(keep, shifted, torch.zeros(()))
                assert 0.2 < 1.0 - keep.float().mean().item() < 0.3
            else:
                want = shifted.cuda()
                lo, hi = aug["scale_range"]
                check(lib().fer_latent_augment(want.data_ptr(), nb, 18 * 512, aug["noise_std"], lo, hi, aug["mask_prob"],
                                               seed, ops.stream()), "latent_augment")
            assert_bits_equal(f"{sorted(aug)} batch {k}", x.cpu(), want.cpu())
    ds.close()


def test_augment_latents_with_directions(tmp_path):
    from data.augment_latents import augment_latents_with_directions

    src, dst = tmp_path / "latents", tmp_path / "augmented"
    src.mkdir()
    g = torch.Generator().manual_seed(8)
    samples = {}
    for i, name in enumerate(["a_001", "b.x_002", "c"]):
        samples[name] = {"latent": torch.randn(18, 512, generator=g), "label": i + 2, "img_path": f"img/{name}.png"}
        torch.save(samples[name], src / f"{name}.pt")
    (src / "notes.txt").write_text("not a sample")
    directions = torch.randn(5, 512, generator=g).numpy()
    indices, steps = [3, 1], [-2.0, -1.0, 1.0, 2.5]
    augment_latents_with_directions(str(src), str(dst), directions, indices, steps)

    want_names = {f"{b}.pt" for b in samples} | {f"{b}_dir{d}_step{s:.1f}.pt" for b in samples for d in indices
                                                 for s in steps}
    assert set(os.listdir(dst)) == want_names and len(want_names) == 3 * (1 + 2 * 4)
    for b, smp in samples.items():
        orig = torch.load(dst / f"{b}.pt", weights_only=False)
        assert set(orig) == {"latent", "label", "img_path"} and orig["label"] == smp["label"]
        assert_bits_equal(b, orig["latent"], smp["latent"])
        for d in indices:
            for s in steps:
                got = torch.load(dst / f"{b}_dir{d}_step{s:.1f}.pt", weights_only=False)
                assert set(got) == {"latent", "label", "augmented", "direction_idx", "step"}
                assert got["label"] == smp["label"] and got["augmented"] is True
                assert got["direction_idx"] == d and got["step"] == s
                ref = smp["latent"] + s * torch.tensor(directions[d], dtype=torch.float32).unsqueeze(0)
                assert got["latent"].dtype == torch.float32 and got["latent"].shape == (18, 512)
                assert_bits_equal(f"{b} dir {d} step {s}", got["latent"], ref)

    # a second run rewrites nothing; a file that went missing comes back, alone
    for n in want_names:
        os.utime(dst / n, ns=(1, 1))
    gone = "c_dir1_step2.5.pt"
    os.remove(dst / gone)
    augment_latents_with_directions(str(src), str(dst), directions, indices, steps)
    assert set(os.listdir(dst)) == want_names
    assert [n for n in want_names if os.stat(dst / n).st_mtime_ns != 1] == [gone]
    back = torch.load(dst / gone, weights_only=False)
    assert_bits_equal("restored", back["latent"], samples["c"]["latent"] + 2.5 * torch.tensor(directions[1]).unsqueeze(0))


def test_augment_shard(tmp_path):
    rng = np.random.default_rng(12)
    n, L, D = 5, 3, 8
    lat = rng.standard_normal((n, L, D), dtype=np.float32)
    lab = rng.integers(0, 7, n)
    paths = [f"p{i}.png" for i in range(n)]
    src, dst = str(tmp_path / "src.fwps"), str(tmp_path / "dst.fwps")
    write_shard(src, lat, lab, paths)
    directions = rng.standard_normal((4, D), dtype=np.float32)
    indices, steps = [2, 0], (-1.0, 0.5, 3.0)
    per = len(indices) * len(steps)
    assert augment_shard(src, dst, directions, indices, steps, block=2) == n * (1 + per)  # 3 blocks, the last short
    ds = PackedLatentDataset(dst)
    assert len(ds) == n * (1 + per) and (ds.L, ds.D) == (L, D)
    got = torch.empty(len(ds), L, D)
    ds.gather(np.arange(len(ds)), got)
    x = torch.from_numpy(lat)
    want = [x] + [(x[i] + s * torch.from_numpy(directions[d]).unsqueeze(0))[None] for i in range(n) for d in indices
                  for s in steps]
    assert_bits_equal("augment_shard latents", got, torch.cat(want))
    assert np.array_equal(ds.labels, np.concatenate([lab, np.repeat(lab, per)]))
    assert list(ds.img_paths()) == paths + [p for p in paths for _ in range(per)]
    ds.close()
    # w+ directions [K, L, D]
    dirs3 = rng.standard_normal((2, L, D), dtype=np.float32)
    assert augment_shard(src, dst, dirs3, [1], (2.0,)) == 2 * n
    ds = PackedLatentDataset(dst)
    got = torch.empty(2 * n, L, D)
    ds.gather(np.arange(2 * n), got)
    assert_bits_equal("w+ directions", got[n:], x + 2.0 * torch.from_numpy(dirs3[1])[None])
    ds.close()
