"""The device step counter (fer_set_step_counter, csrc/step_seed.h) reaches every code object that has a
dropout kernel. Each .hip file is its own code object with its own copy of the counter pointer; a file that
includes step_seed.h registers its setter when the library loads, and a file whose pointer were never set
would replay identical masks under fervit.graph.StepGraph without any error.

This test does NOT enumerate code objects: it calls one entry point per file that includes step_seed.h
(CASES below). Whoever adds a file with a dropout kernel adds a line there.

Per entry point, eagerly (no graph capture), at the smallest shape its host checks accept, p = 0.5 and a
fixed host seed:
  * with a device uint64 counter registered, the output at counter value 0 differs from the one at value 1;
  * with the counter unregistered, two calls are bit-equal."""
import pytest
import torch

from elemwise import assert_bits_equal
from fervit import ops
from fervit._lib import check, lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
P, SEED = 0.5, 0x5EED0123456789
M = C = 64
BF16 = torch.bfloat16


def rnd(*shape, dtype=torch.float32, salt=0):
    g = torch.Generator().manual_seed(1234 + salt)
    return torch.randn(*shape, generator=g).to(DEV, dtype)


def gemm_case():  # csrc/gemm.hip: epilogue dropout, bf16, K = 64
    a, b = rnd(M, 64, dtype=BF16), rnd(C, 64, dtype=BF16, salt=1)
    return lambda: ops.gemm(a, b, torch.empty(M, C, dtype=BF16, device=DEV), M=M, N=C, K=64, dropout=P, seed=SEED)


def attention_case():  # csrc/attention.hip: one head of dh = 64 over 8 tokens, dropout on the probabilities
    B, N, H, dh = 1, 8, 1, 64
    qkv = rnd(B * N, 3 * H * dh, dtype=BF16)
    saved = ops.attention_saved(qkv, B, N, H, dh, dropout=P)
    return lambda: ops.attention_fwd(qkv, torch.empty(B * N, H * dh, dtype=BF16, device=DEV), saved, B, N, H, dh,
                                     dropout=P, seed=SEED)


def layernorm_case():  # csrc/layernorm.hip: layernorm_bwd's dx_drop
    x, dy, w, b = rnd(M, C), rnd(M, C, salt=1), rnd(C, salt=2), rnd(C, salt=3)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x, w, b, 1e-5, mean=mean, rstd=rstd)

    def run():
        dxd = torch.empty(M, C, device=DEV)
        ops.layernorm_bwd(dy, x, mean, rstd, w, dx_drop=dxd, dropout=P, seed=SEED)
        return dxd
    return run


def batchnorm_case():  # csrc/convbn.hip
    x, gamma, beta = rnd(M, C), rnd(C, salt=1), rnd(C, salt=2)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    return lambda: ops.batchnorm_fwd(x, gamma, beta, rm, rv, nbt, True, dropout=P, seed=SEED)[0]


def relu_dropout_case():  # csrc/attnpool.hip
    x = rnd(M, C)
    return lambda: ops.relu_dropout_fwd(x, dropout=P, seed=SEED)


def pool2_chdrop_case():  # csrc/conv2d.hip: Dropout2d, one keep bit per (sample, channel)
    B, H, W = 1, 8, 8
    x = rnd(B * H * W, C)
    return lambda: ops.pool2_chdrop_fwd(x, B, H, W, True, dropout=P, seed=SEED)


def tokens_case():  # csrc/vit_edge.hip
    B, n = 8, 7
    emb, cls, pos = rnd(B * n, C), rnd(C, salt=1), rnd((n + 1) * C, salt=2)
    return lambda: ops.tokens_fwd(emb, cls, pos, B, n, C, dropout=P, seed=SEED)


def latent_augment_case():  # csrc/wplus.hip: the mask stage alone, mask_prob = p (in place)
    x = rnd(M, C)

    def run():
        y = x.clone()
        check(lib().fer_latent_augment(y.data_ptr(), M, C, 0.0, 1.0, 1.0, P, ops.seed64(SEED), ops.stream()),
              "latent_augment")
        return y
    return run


def dropout_case():  # csrc/optim.hip
    x = rnd(M, C)
    return lambda: ops.dropout(x, P, SEED)


CASES = {
    "gemm": gemm_case,
    "attention_fwd": attention_case,
    "layernorm_bwd": layernorm_case,
    "batchnorm_fwd": batchnorm_case,
    "relu_dropout_fwd": relu_dropout_case,
    "pool2_chdrop_fwd": pool2_chdrop_case,
    "tokens_fwd": tokens_case,
    "latent_augment": latent_augment_case,
    "dropout": dropout_case,
}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                       b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_step_counter_reaches_code_object(name):
    run = CASES[name]()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)  # the ABI's uint64_t
    try:
        check(lib().fer_set_step_counter(counter.data_ptr()), "set_step_counter")
        at0 = run()
        counter.fill_(1)
        at1 = run()
        assert not same_bits(at0, at1), f"{name}: the same output at step 0 and step 1 (counter not seen)"
        check(lib().fer_set_step_counter(None), "set_step_counter")
        assert_bits_equal(f"{name} without a counter, two calls", run(), run())
    finally:
        check(lib().fer_set_step_counter(None), "set_step_counter")
        torch.cuda.synchronize()
