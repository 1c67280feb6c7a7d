"""The KV-cache attention kernels of csrc/attention.hip that promise one another's bits, held to it.  launch_attention sends a depth sub-step with few
queries over a short cache to attention_fewq_kernel (one wave per (sample, head), one softmax group of attention_kernel per query) and, at head size 64
from 64 samples, to attention_fewq8_kernel (eight heads per wave, the sums in fewq's tree order); HQT_NO_FEWQ8=1 and HQT_NO_FEWQ_ATTN=1 switch each
off.  EXACT's "a row's draws do not depend on the pass it sits in" rests on the three computing the same bits.

The switches are read once per process, so every leg is a fresh child process, one after another: it builds one engine, runs two positions teacher-forced on
fixed codes and saves the logits; the legs of a case are then compared byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ('HQT_NO_FEWQ_ATTN', 'HQT_NO_FEWQ8')

CHILD = """
import json, sys, numpy as np, torch
sys.path.insert(0, %r)
from hqtransformer_amd import synth
from hqtransformer_amd._lib import PRECISIONS
from hqtransformer_amd.engine import Engine
from hqtransformer_amd.spec import Stage2Spec
case = json.loads(sys.argv[1])
spec = Stage2Spec(**case['spec'])
B, n, L = case['B'], 2, 3 if case['spec'].get('levels') == 3 else 2
eng = Engine(spec, None, torch.device('cuda:0'), B, spec.ctx_len_img)
eng.load(stage2=synth.stage2_weights(spec, case['seed'], 'fixture'))
eng.finalize()
r = np.random.default_rng(case['seed'] + 1)
force = [torch.from_numpy(r.integers(0, spec.vocab_top, (B, n) + ((4 ** l,) if l else ()))) for l in range(L)]
cond = torch.from_numpy(np.arange(B) %% spec.n_classes)
kw = dict(precision=PRECISIONS[case['precision']], seed=5, return_logits=True, use_graph=False)
if L == 3:
    lg = eng.sample3(B, cond, n, force=force, **kw)[3]
else:
    lg = eng.sample(B, cond, n, force_top=force[0], force_bot=force[1], **kw)[2]
torch.cuda.synchronize()
eng.range_check()
assert bool(torch.isfinite(lg).all())
np.save(sys.argv[2], lg.cpu().numpy())
""" % ROOT

# head size 64, one body and one depth layer: depth sub-step 1 is 4 queries over 5 keys
SPEC_A = dict(embed_dim=128, n_layers=1, n_heads=2, n_layers_depth=1, vocab_top=512, vocab_bot=512, vocab_txt=64, ctx_len_img=16, ctx_len_txt=16,
              n_classes=10, cond=1, embedding=0)
# three levels, head size 32 (the tiny-l3 geometry): sub-step 2 is 16 queries over 21 keys, two passes of 16 rows
SPEC_B = dict(SPEC_A, n_heads=4, levels=3)


def run_legs(tmp_path, case, legs):
    """{leg: logits}; stops at the first child that does not exit 0"""
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    out = {}
    for leg, env in legs.items():
        path = str(tmp_path / f'{leg}.npy')
        rr = subprocess.run([sys.executable, '-c', CHILD, json.dumps(case), path], cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=120)
        assert rr.returncode == 0, (leg, rr.returncode, rr.stdout[-1500:], rr.stderr[-1500:])
        out[leg] = np.load(path)
    return out


def assert_same_bits(out):
    first, *rest = out
    for leg in rest:
        assert out[leg].shape == out[first].shape and out[leg].dtype == out[first].dtype
        same = np.array_equal(out[leg].view(np.uint8), out[first].view(np.uint8))
        print(f'{leg} vs {first}: largest difference {np.abs(out[leg] - out[first]).max()}')
        assert same, f'the logits of leg {leg} differ from those of leg {first}'


@pytest.mark.parametrize('precision', ['exact', 'fast'])
def test_eight_heads_per_wave_one_head_per_wave_and_one_wave_per_query_agree(tmp_path, precision):
    """B = 64 at head size 64: attention_fewq8_kernel<., 5, 4> by default, attention_fewq_kernel<., 1> without fewq8, attention_kernel without both."""
    out = run_legs(tmp_path, dict(spec=SPEC_A, B=64, seed=301, precision=precision),
                   {'fewq8': {}, 'fewq': {'HQT_NO_FEWQ8': '1'}, 'per_query': {'HQT_NO_FEWQ_ATTN': '1'}})
    assert_same_bits(out)


def test_two_pass_group_one_head_per_wave_and_one_wave_per_query_agree(tmp_path):
    """B = 3 at head size 32, EXACT: attention_fewq_kernel<float, 2> by default, attention_kernel without it."""
    out = run_legs(tmp_path, dict(spec=SPEC_B, B=3, seed=311, precision='exact'), {'fewq': {}, 'per_query': {'HQT_NO_FEWQ_ATTN': '1'}})
    assert_same_bits(out)
