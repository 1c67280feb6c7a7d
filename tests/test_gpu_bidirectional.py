"""The bidirectional depth head (hqt_config.depth_decoding = 4, iHQGPT model_type 'bidirectional4', hierarchical_ar.py:791-878) through the
C ABI against fixture G13, generated from the reference by tools/gen_golden_bidir.py.  Per top position the depth blocks run ONCE, unmasked,
over [ln_f(h) + sos_depth, pos_emb_depth[0..3]]; all five draws use temperature[0], top_k_bot and top_p_bot (the reference's own choice),
so the fixture's two settings give top and bottom different k / p / T.  Bars as in tests/test_gpu_parity.py: EXACT codes bit-exact and
logits within 2e-4 (the reference logs post-temperature logits, the engine pre-temperature ones: T[0] in all five slots); FAST teacher-
forced logits within the two-level FAST gate of that file."""
import json
import os

import numpy as np
import pytest
import torch

from hqtransformer_amd import _lib, synth
from hqtransformer_amd._lib import PRECISION_EXACT, PRECISION_FAST, PRECISION_SPLIT
from hqtransformer_amd.config import load_config
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.spec import Stage2Spec
from tests.helpers import gate, load

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def engine_s2(spec, weights, max_batch, max_steps=None, poison=False):
    if poison:                       # every workspace buffer starts as NaN: an unwritten row or an out-of-bounds write shows up
        os.environ['HQT_POISON_WORKSPACE'] = '1'
    try:
        e = Engine(spec, None, dev(), max_batch, max_steps or spec.ctx_len_img)
    finally:
        os.environ.pop('HQT_POISON_WORKSPACE', None)
    e.load(stage2=weights)
    e.finalize()
    return e


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def g13():
    fx = load('g13_tiny_cls_bidirectional.npz')
    spec = Stage2Spec(**json.loads(str(fx['spec'])))
    weights = synth.stage2_weights(spec, int(fx['weight_seed']), 'fixture')
    return fx, spec, weights, engine_s2(spec, weights, 16)


def _run(fx, spec, eng, si, precision, graph, n=None):
    tk, tp, T = json.loads(str(fx['settings']))[si]
    B, n = int(fx['B']), n or int(fx['n_steps'])
    noise = synth.exp_noise(int(fx['noise_seed']), int(fx['n_steps']), B, spec.vocab_top)[:n]
    return eng.sample(B, torch.full((B,), int(fx['cond'])), n, precision=precision, top_k=tk, top_p=tp, temperature=T,
                      noise=torch.from_numpy(noise.copy()), return_logits=True, use_graph=graph), T


@pytest.mark.parametrize('si', [0, 1])
@pytest.mark.parametrize('graph', [False, True])
def test_exact_codes_bit_exact_vs_reference_fixture(g13, si, graph):
    fx, spec, _, eng = g13
    (ct, cb, lg), T = _run(fx, spec, eng, si, PRECISION_EXACT, graph)
    torch.cuda.synchronize()
    err = np.abs(np_(lg)[fx['keep_steps']] / np.float32(T[0]) - fx[f'logits_{si}']).max()
    assert err <= LOGIT_TOL, f'logit error {err}'
    assert (np_(ct) == fx[f'codes_top_{si}']).all(), 'top codes differ from the reference'
    assert (np_(cb) == fx[f'codes_bot_{si}']).all(), 'bottom codes differ from the reference'


def test_exact_reduce_uncond_vs_reference_fixture(g13):
    fx = g13[0]
    spec = Stage2Spec(**json.loads(str(fx['reduce_spec'])))
    eng = engine_s2(spec, synth.stage2_weights(spec, int(fx['reduce_weight_seed']), 'fixture'), 4)
    B, n = int(fx['B']), int(fx['reduce_n_steps'])
    tk, tp, T = json.loads(str(fx['reduce_setting']))
    noise = synth.exp_noise(int(fx['reduce_noise_seed']), n, B, spec.vocab_top)
    for graph in (False, True):
        ct, cb, lg = eng.sample(B, None, n, precision=PRECISION_EXACT, top_k=tk, top_p=tp, temperature=T, noise=torch.from_numpy(noise),
                                return_logits=True, use_graph=graph)
        assert np.abs(np_(lg)[fx['reduce_keep_steps']] / np.float32(T[0]) - fx['reduce_logits']).max() <= LOGIT_TOL
        assert (np_(ct) == fx['reduce_codes_top']).all() and (np_(cb) == fx['reduce_codes_bot']).all()


@pytest.mark.parametrize('si', [0, 1])
def test_split_codes_bit_exact_vs_reference_fixture(g13, si):
    fx, spec, _, eng = g13
    (ct, cb, _), _ = _run(fx, spec, eng, si, PRECISION_SPLIT, False)
    eng.range_check()
    assert (np_(ct) == fx[f'codes_top_{si}']).all() and (np_(cb) == fx[f'codes_bot_{si}']).all()


def test_fast_teacher_forced_vs_exact(g13):
    """FAST fed the reference's codes (force_top / force_bot replace what the next position's spatial embedding reads; the depth pass of
    this head reads no code): logits against EXACT within the two-level FAST gate (0.15), drawn codes >= 96 % the same."""
    fx, spec, _, eng = g13
    B, n = int(fx['B']), 16
    noise = torch.from_numpy(synth.exp_noise(int(fx['noise_seed']), int(fx['n_steps']), B, spec.vocab_top)[:n].copy())
    ft = torch.from_numpy(fx['codes_top_0'][:, :n].copy())
    fb = torch.from_numpy(fx['codes_bot_0'][:, :n].copy())
    cond = torch.full((B,), int(fx['cond']))
    ex = eng.sample(B, cond, n, precision=PRECISION_EXACT, noise=noise, force_top=ft, force_bot=fb, return_logits=True, use_graph=False)
    for graph in (False, True):
        ct, cb, lg = eng.sample(B, cond, n, precision=PRECISION_FAST, noise=noise, force_top=ft, force_bot=fb, return_logits=True, use_graph=graph)
        eng.range_check()
        gate(f'bidir_tiny.fast_logits(graph={graph})', (lg - ex[2]).abs().max().item(), 0.15)
        agree = ((ct == ex[0]).float().mean().item() + (cb == ex[1]).float().mean().item()) / 2
        gate(f'bidir_tiny.fast_code_agreement(graph={graph})', agree, 0.96, '>=')


def test_merged_pass_equals_step_at_a_time_exact(g13):
    """Three steps (own class, Philox seed and row offset each) as ONE pass of 3 B rows (hqt_sample_opts.row_seeds / row_offsets): in EXACT
    every row draws what it draws in its own call."""
    _, spec, _, eng = g13
    B, n = 4, 12
    steps = [(5, 11, 0), (2, 12, 64), (9, 13, 7)]          # (class id, seed, sample_offset)
    kw = dict(precision=PRECISION_EXACT, top_k=(None, 100), top_p=(None, 0.95), temperature=(1.1, 0.8))
    sep = [eng.sample(B, torch.full((B,), c), n, seed=s, sample_offset=o, use_graph=False, **kw) for c, s, o in steps]
    cond = torch.cat([torch.full((B,), c) for c, _, _ in steps])
    seeds = [s for _, s, _ in steps for _ in range(B)]
    offs = [o + b for _, _, o in steps for b in range(B)]
    for graph in (False, True):
        mt, mb = eng.sample(3 * B, cond, n, row_seeds=seeds, row_offsets=offs, use_graph=graph, **kw)
        for i, (ct, cb) in enumerate(sep):
            assert torch.equal(mt[i * B:(i + 1) * B], ct) and torch.equal(mb[i * B:(i + 1) * B], cb), f'merged step {i} (graph={graph})'


@pytest.mark.parametrize('B', [20, 50])
def test_padded_batch_equals_its_unpadded_rows(B):
    """5 B depth rows whose packed row block is wider than round32(5 B) (B = 20: 100 rows in 128, B = 50: 250 in 256) on a NaN-poisoned
    workspace: EXACT rows equal the rows of a 3-sample call; FAST teacher-forced logits finite and within the FAST gate of EXACT."""
    spec = Stage2Spec(embed_dim=256, n_layers=2, n_heads=4, n_layers_depth=2, vocab_top=512, vocab_bot=512, vocab_txt=64,
                      ctx_len_img=64, ctx_len_txt=16, n_classes=10, cond=1, embedding=0, depth_decoding='bidirectional')
    weights = synth.stage2_weights(spec, 211, 'fixture')
    n = 4
    noise = synth.exp_noise(212, n, B, spec.vocab_top)
    cond = torch.from_numpy(np.arange(B) % spec.n_classes)
    eng = engine_s2(spec, weights, B, 8, poison=True)
    kw = dict(top_k=(None, 64), top_p=(None, 0.9), temperature=(0.9, 1.2), return_logits=True, use_graph=False)
    ct, cb, lg = eng.sample(B, cond, n, precision=PRECISION_EXACT, noise=torch.from_numpy(noise), **kw)
    assert bool(torch.isfinite(lg).all())
    st, sb, sl = eng.sample(3, cond[:3], n, precision=PRECISION_EXACT, noise=torch.from_numpy(noise[:, :, :3].copy()), **kw)
    assert torch.equal(st, ct[:3]) and torch.equal(sb, cb[:3]) and torch.equal(sl, lg[:, :, :3])
    for graph in (False, True):
        kw['use_graph'] = graph
        _, _, lf = eng.sample(B, cond, n, precision=PRECISION_FAST, noise=torch.from_numpy(noise), force_top=ct, force_bot=cb, **kw)
        eng.range_check()
        assert bool(torch.isfinite(lf).all()), f'NaN logits at B={B} (graph={graph})'
        gate(f'bidir_padded{B}.fast_logits(graph={graph})', (lf - lg).abs().max().item(), 0.15)


def test_persistent_body_on_and_off(g13):
    """FAST decode steps of up to 64 samples run the body as one persistent launch (persist_body); the whole-position launch of the
    'parallel' head (persist_position) never runs for this head.  Teacher-forced, the persistent body and the launch chain draw the
    same codes (both bf16, different summation orders: held to the FAST gates against each other and against EXACT)."""
    fx, spec, _, eng = g13
    B, n = 8, 8
    noise = torch.from_numpy(synth.exp_noise(41, n, B, spec.vocab_top))
    cond = torch.from_numpy(np.arange(B) % spec.n_classes)
    kw = dict(noise=noise, top_k=(8, 64), top_p=(0.5, 0.9), temperature=(0.9, 1.3), return_logits=True, use_graph=False)
    ct, cb, lg_e = eng.sample(B, cond, n, precision=PRECISION_EXACT, **kw)
    runs = {}
    for on in (True, False):
        eng.set_persist(on)
        try:
            eng.timing_reset()
            eng.timing(True)
            runs[on] = eng.sample(B, cond, n, precision=PRECISION_FAST, force_top=ct, force_bot=cb, **kw)
            eng.range_check()
            rep = eng.timing_report()
            eng.timing(False)
        finally:
            eng.set_persist(True)
        assert 'persist_position' not in rep or rep['persist_position'][0] == 0, rep
        assert rep.get('persist_body', (0,))[0] == (n if on else 0), rep
        for name in ('bidir_depth_input', 'bidir_head_ln', 'bidir_sampler_top', 'bidir_sampler_bot'):
            assert rep[name][0] == n, (name, rep)
        assert rep['gemm_head'][0] == 2 * n and rep['gemm_qkv'][0] == (0 if on else spec.n_layers * n) + spec.n_layers_depth * n, rep
    (pt, pb, lp), (qt, qb, lq) = runs[True], runs[False]
    gate('bidir_tiny.persist_vs_chain_logits', (lp - lq).abs().max().item(), 0.15)
    gate('bidir_tiny.persist_vs_exact_logits', (lp - lg_e).abs().max().item(), 0.15)
    agree = ((pt == qt).float().mean().item() + (pb == qb).float().mean().item()) / 2
    gate('bidir_tiny.persist_vs_chain_code_agreement', agree, 0.96, '>=')


def test_surface_samples_and_refuses_given_top_code():
    """ImageGPT2 / sampling_ihqgpt on a bidirectional config; given_top_code, which the reference ignores for this head, raises."""
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.sampling import sampling_ihqgpt
    model = ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml'), ['stage2.type=hq-transformer/bidirectional4']), seed=5).to('cuda').eval()
    assert model.stage2.model_type == 'bidirectional'
    ct, cb = sampling_ihqgpt(model.stage2, num_candidates=2, cond=3, top_k_top=16, top_k_bot=32, softmax_temperature=[1.0, 0.9],
                             use_fp16=True, is_tqdm=False, max_seq_len=8, seed=5)
    model.stage2.range_check()
    assert ct.shape == (2, 8) and cb.shape == (2, 8, 4) and int(ct.max()) < 512 and int(cb.min()) >= 0
    with pytest.raises(ValueError, match='given_top_code'):
        sampling_ihqgpt(model.stage2, num_candidates=2, cond=3, max_seq_len=8, given_top_code=torch.zeros(2, 8, dtype=torch.int64))


def test_create_refuses_bidirectional_with_three_levels_or_text():
    base = dict(embed_dim=128, n_layers=1, n_heads=4, n_layers_depth=1, vocab_top=512, vocab_bot=512, vocab_txt=64, ctx_len_img=16,
                ctx_len_txt=16, n_classes=10, cond=1, embedding=0)
    Engine(Stage2Spec(**base, depth_decoding='bidirectional'), None, dev(), 2, 4)        # two levels: accepted
    with pytest.raises(_lib.HqtError):
        Engine(Stage2Spec(**base, levels=3, depth_decoding='bidirectional'), None, dev(), 2, 4)
    with pytest.raises(_lib.HqtError):
        Engine(Stage2Spec(**dict(base, cond=2, n_classes=0), depth_decoding='bidirectional'), None, dev(), 2, 4)
