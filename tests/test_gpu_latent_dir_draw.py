"""fer_latent_dir_draw (csrc/wplus.hip) element for element against its host replica (latent_dirs_ref.dir_draw:
integer hashes, one float32 comparison), and the device step counter for this entry alone, the two assertions
tests/test_gpu_step_counter.py makes per code object."""
import numpy as np
import pytest
import torch

import latent_dirs_ref as R
from abi_harness import DEV, last_error, lib
from fervit import ops
from fervit._lib import check

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789


@pytest.mark.parametrize("p_keep", [0.0, 1.0 / 17.0, 1.0])
@pytest.mark.parametrize("n_choices", [1, 16, 40])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_draw_equals_replica(n, n_choices, p_keep):
    buf = torch.full((n + 8,), -7, dtype=torch.int32, device=DEV)
    got = ops.latent_dir_draw(n, n_choices, p_keep, SEED + n, out=buf[4:4 + n])
    ref = R.dir_draw(SEED + n, n, n_choices, p_keep)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert (buf[:4] == -7).all() and (buf[4 + n:] == -7).all()
    if p_keep == 0.0:
        assert ref.min() >= 0
    if p_keep == 1.0:
        assert (ref == -1).all()
    if n == 5000 and p_keep == 1.0 / 17.0 and n_choices > 1:
        assert (ref == -1).any() and len(np.unique(ref)) == n_choices + 1


def test_step_counter_reaches_the_draw():
    n, nc, p = 4096, 16, 1.0 / 17.0
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    try:
        check(lib().fer_set_step_counter(counter.data_ptr()), "set_step_counter")
        at0 = ops.latent_dir_draw(n, nc, p, SEED)
        counter.fill_(1)
        at1 = ops.latent_dir_draw(n, nc, p, SEED)
        assert not torch.equal(at0, at1), "the same draw at step 0 and step 1 (counter not seen)"
        check(lib().fer_set_step_counter(None), "set_step_counter")
        a, b = ops.latent_dir_draw(n, nc, p, SEED), ops.latent_dir_draw(n, nc, p, SEED)
        assert torch.equal(a, b)
        assert np.array_equal(a.cpu().numpy(), R.dir_draw(SEED, n, nc, p))
    finally:
        check(lib().fer_set_step_counter(None), "set_step_counter")
        torch.cuda.synchronize()


def test_argument_errors():
    out = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    L = lib()
    for nc, p in ((0, 0.5), (-1, 0.5), (4, -0.1), (4, 1.5), (4, float("nan"))):
        rc = L.fer_latent_dir_draw(out.data_ptr(), 4, nc, p, SEED, ops.stream())
        assert rc != 0 and last_error().startswith("latent_dir_draw:"), (nc, p, last_error())
    assert L.fer_latent_dir_draw(out.data_ptr(), 2 ** 31, 4, 0.5, SEED, ops.stream()) != 0
    assert L.fer_latent_dir_draw(out.data_ptr(), 0, 4, 0.5, SEED, ops.stream()) == 0
    torch.cuda.synchronize()
    assert (out == -7).all()
