"""Plain restatement of ``TransformerOracle.forward``
(tracktolearn_amd/oracles/transformer_oracle.py), op by op, with switches.

TEST INFRASTRUCTURE ONLY.  Nothing in the package imports this file.

``forward(params(model), x)`` is the network in float64: embedding, CLS,
positional encoding, per-head attention, post-norm encoder layers, head,
sigmoid.  It does not call ``nn.TransformerEncoder``; it is the truth the
fused kernels (csrc/ttl_oracle_net.hip) are judged against.

``emulate_fp16=True`` computes in ``dtype`` and rounds to fp16 at exactly the
points the kernel's header and oracles/fused_net.py document -- the kernel's
stated arithmetic without its summation order:

* inputs, CLS token, embedding weights and bias: fp16; the embedding Linear's
  output fp16, ReLU, times fp16(sqrt 32) rounded to fp16; the positional table
  is added unrounded;
* every Linear (Q, K, V, out-projection, both feed-forward layers, head):
  fp16 operands (the activation is rounded where it enters the product), an
  unrounded sum, the bias added unrounded (the packed vectors are float32;
  only the head's bias is fp16), the result rounded to fp16;
* scores K.Q unrounded; softmax unrounded, as 2^((s - max) log2(e) / sqrt(dh))
  with the scale applied to the difference; P rounded to fp16 after
  normalisation; the attention output P.V rounded to fp16 where it enters the
  out-projection;
* residual sums and LayerNorm unrounded;
* sigmoid unrounded, the score rounded to fp16.

``acc=torch.float32`` runs the same emulation with float32 sums (a twin: what
another summation order and float32 intermediates may legitimately do).

Mutants (``mutant=(name, ...)``): small named deviations a plausible kernel
bug would produce.  The key bias b_k has no mutant: it adds the same constant
q.b_k to all of a query's scores, which softmax cancels -- omitting it is
mathematically invisible.  Likewise the query bias matters (it weights the
keys) but is not listed by itself; the listed bias mutants are those of b_v,
b_o, b_1, b_2 and the LayerNorm gains / biases.
"""
import copy
import math

import torch

D, TOKENS, TILE = 32, 128, 32


def params(model):
    """The module's parameters as a plain dict of float64 CPU tensors."""
    g = lambda t: t.detach().double().cpu()
    layers = []
    for layer in model.bert.layers:
        at = layer.self_attn
        w_in, b_in = g(at.in_proj_weight), g(at.in_proj_bias)
        layers.append({
            'w_q': w_in[0:32], 'w_k': w_in[32:64], 'w_v': w_in[64:96],
            'b_q': b_in[0:32], 'b_k': b_in[32:64], 'b_v': b_in[64:96],
            'w_o': g(at.out_proj.weight), 'b_o': g(at.out_proj.bias),
            'w_1': g(layer.linear1.weight), 'b_1': g(layer.linear1.bias),
            'w_2': g(layer.linear2.weight), 'b_2': g(layer.linear2.bias),
            'g1': g(layer.norm1.weight), 'be1': g(layer.norm1.bias),
            'g2': g(layer.norm2.weight), 'be2': g(layer.norm2.bias),
            'eps': float(layer.norm1.eps)})
    return {'layers': layers, 'n_head': model.bert.layers[0].self_attn.num_heads,
            'w_e': g(model.embedding[0].weight), 'b_e': g(model.embedding[0].bias),
            'cls': g(model.cls_token), 'pe': g(model.pos_encoding.pe[:TOKENS, 0]),
            'w_h': g(model.head.weight)[0], 'b_h': g(model.head.bias)[0]}


def mutants(n_layers, n_head, ff, keys=range(TOKENS), chunks=None):
    """The mutant list of a configuration.  Layers: the first and the last for
    the per-key mutants (the all-tiles path and the token-tile-0 path), every
    layer for the rest."""
    last = n_layers - 1
    out = []
    for l in sorted({0, last}):
        out += [('drop_key', l, j) for j in keys]
    for l in range(n_layers):
        out += [('zero_head', l, h) for h in range(n_head)]
        # (one head: there is nothing to swap with)
        out += [('swap_head', l, h) for h in range(n_head - 1)]
        out += [('skip_ff_chunk', l, c) for c in (range(ff // 32) if chunks is None else chunks)]
        # the last layer updates token tile 0 only: a stale tile 1..3 there is the design
        out += [('stale_tile', l, w) for w in (range(4) if l < last else range(1))]
        out += [('omit', l, v) for v in ('b_v', 'b_o', 'b_1', 'b_2', 'g1', 'be1', 'g2', 'be2')]
        out += [('skip_round', l, v) for v in ('q', 'k', 'v', 'attn', 'o', 'ff1', 'ff2')]
    if n_layers > 1:
        out += [('stale_kv_last', w) for w in range(4)]
    out += [('shift_pe', w) for w in range(4)]
    return out


def _layer_norm(x, g, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b


def forward(p, x, dtype=torch.float64, emulate_fp16=False, acc=None, mutant=None, trace=None):
    """(score, logit) of segment vectors x (N, 127, 3), each (N,) in ``dtype``
    (or ``acc`` when given: the dtype of every sum and intermediate).  A list
    given as ``trace`` receives, per layer, the largest attention weight of
    each key over heads and queries, and over heads for query 0: 2 x (N, 128)."""
    dt = acc if acc is not None else dtype
    mut = mutant if mutant is not None else ('none',)
    name = mut[0]

    def r16(t, what=None):
        """Round to fp16 (emulation only); ``what`` names a Linear's output."""
        if not emulate_fp16 or (what is not None and mut == ('skip_round', what[0], what[1])):
            return t
        return t.to(torch.float16).to(dt)

    c = lambda t: t.to(dt)
    n = x.shape[0]
    n_head = p['n_head']
    dh = D // n_head
    n_layers = len(p['layers'])

    # ---- embedding of [CLS, segments], scaled, plus the positional table
    seq = torch.cat([c(p['cls']).expand(n, 1, 3), c(x)], dim=1)              # (N, 128, 3)
    e = r16(r16(seq) @ r16(c(p['w_e'])).T + r16(c(p['b_e'])))
    e = torch.relu(e)
    e = r16(e * r16(torch.tensor(math.sqrt(D), dtype=dt)))
    pe = c(p['pe'])
    if name == 'shift_pe':
        t0 = TILE * mut[1]
        idx = torch.arange(TOKENS)
        idx[t0:t0 + TILE] = (idx[t0:t0 + TILE] + 1).clamp(max=TOKENS - 1)
        if mut[1] == 3:         # (the table has 128 rows here: the last token takes the formula's)
            pe = torch.cat([pe, _pe_row(TOKENS).to(dt).view(1, D)])
            idx[TOKENS - 1] = TOKENS
        pe = pe[idx]
    h = e + pe

    k_prev = v_prev = None
    for l, L in enumerate(p['layers']):
        last = l == n_layers - 1
        here = len(mut) > 1 and mut[1] == l
        W = lambda key: r16(c(L[key]))
        bias = lambda key: 0.0 if (name == 'omit' and here and mut[2] == key) else c(L[key])
        gain = lambda key: 1.0 if (name == 'omit' and here and mut[2] == key) else c(L[key])
        h_in = h
        h16 = r16(h)
        q = r16(h16 @ W('w_q').T + c(L['b_q']), (l, 'q'))
        k = r16(h16 @ W('w_k').T + c(L['b_k']), (l, 'k'))
        v = r16(h16 @ W('w_v').T + bias('b_v'), (l, 'v'))
        if name == 'stale_kv_last' and last:
            sl = slice(TILE * mut[1], TILE * mut[1] + TILE)
            k, v = k.clone(), v.clone()
            k[:, sl], v[:, sl] = k_prev[:, sl], v_prev[:, sl]
        k_prev, v_prev = k, v

        # ---- attention, head by head
        heads = []
        for hd in range(n_head):
            f = slice(dh * hd, dh * hd + dh)
            s = q[:, :, f] @ k[:, :, f].transpose(1, 2)                       # (N, query, key)
            if name == 'drop_key' and here:
                s = s.clone()
                s[:, :, mut[2]] = -math.inf
            m = s.max(-1, keepdim=True).values
            if emulate_fp16:
                num = torch.exp2((s - m) * (c(torch.tensor(1.4426950408889634)) / math.sqrt(dh)))
            else:
                num = torch.exp((s - m) / math.sqrt(dh))
            prob = r16(num / num.sum(-1, keepdim=True))
            heads.append(prob @ v[:, :, f])
            if trace is not None:
                seen = (prob.max(1).values, prob[:, 0])
                if hd == 0:
                    trace.append(seen)
                else:
                    trace[l] = tuple(torch.maximum(a, b) for a, b in zip(trace[l], seen))
        if name == 'zero_head' and here:
            heads[mut[2]] = torch.zeros_like(heads[mut[2]])
        if name == 'swap_head' and here:
            a, b = mut[2], mut[2] + 1
            heads[a], heads[b] = heads[b], heads[a]
        attn = r16(torch.cat(heads, dim=-1), (l, 'attn'))
        o = r16(attn @ W('w_o').T + bias('b_o'), (l, 'o'))
        h = _layer_norm(h + o, gain('g1'), bias('be1'), L['eps'])

        # ---- feed-forward block
        w1, b1, w2 = W('w_1'), bias('b_1'), W('w_2')
        f1 = torch.relu(r16(r16(h) @ w1.T + b1, (l, 'ff1')))
        if name == 'skip_ff_chunk' and here:
            f1 = f1.clone()
            f1[:, :, 32 * mut[2]:32 * mut[2] + 32] = 0
        f2 = r16(f1 @ w2.T + bias('b_2'), (l, 'ff2'))
        h = _layer_norm(h + f2, gain('g2'), bias('be2'), L['eps'])

        if name == 'stale_tile' and here:
            sl = slice(TILE * mut[2], TILE * mut[2] + TILE)
            h = h.clone()
            h[:, sl] = h_in[:, sl]

    logit = r16(r16(h[:, 0]) @ r16(c(p['w_h'])) + r16(c(p['b_h'])))
    score = r16(torch.sigmoid(logit))
    return score, logit


def _pe_row(t):
    """Row t of the sinusoidal table (transformer_oracle.py:PositionalEncoding)."""
    div = torch.exp(torch.arange(0, D, 2, dtype=torch.float32) * (-math.log(10000.0) / D))
    row = torch.zeros(D, dtype=torch.float32)
    row[0::2] = torch.sin(t * div)
    row[1::2] = torch.cos(t * div)
    return row.double()


# --------------------------------------------------------------------------
# Row tolerance from twins of the emulation (tests/test_oracle_net_reference.py)
# --------------------------------------------------------------------------
def fp16_ulp(score):
    """Spacing of fp16 at ``score`` in (0, 1): 2^(floor(log2 s) - 10), at least the
    subnormal spacing 2^-24 (4.9e-4 in [0.5, 1), less below)."""
    s = score.double().abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(s)) - 10)


def ulp_moved(x, seed):
    """x with every element moved by one float32 ulp, up or down (seeded)."""
    x = x.float()
    g = torch.Generator().manual_seed(seed)
    up = torch.rand(x.shape, generator=g) < 0.5
    return torch.where(up, torch.nextafter(x, torch.full_like(x, math.inf)),
                       torch.nextafter(x, torch.full_like(x, -math.inf)))


def autocast_twin(model, x, device='cpu'):
    """The ``nn`` module under ``torch.autocast(fp16)``: on the GPU what the
    reference runs, on the CPU its stand-in (same rounding points, other sums)."""
    model = copy.deepcopy(model).float().to(device)
    with torch.no_grad(), torch.autocast(device, dtype=torch.float16):
        return model(x.float().to(device)).double().cpu()


def cpu_twins(model, p, x):
    """Scores of the CPU twins of the emulation: float32 sums, inputs moved by
    one float32 ulp, the module under CPU autocast.  [(name, scores float64)]."""
    return [('float32 sums', forward(p, x, emulate_fp16=True, acc=torch.float32)[0].double()),
            ('inputs + 1 ulp', forward(p, ulp_moved(x, 5), emulate_fp16=True)[0]),
            ('autocast (cpu)', autocast_twin(model, x))]


def logit_rounding_fits(score, logit):
    """Whether one fp16 ulp of the logit moves the score by at most one fp16 ulp
    of the score: ulp16(y) s (1 - s) <= ulp16(s).  The head is a Linear, so its
    output -- the logit -- is rounded to fp16 before the sigmoid, and ANY
    legitimate difference upstream (one of the ~10^5 fp16 roundings of a row
    landing on the other side: the float32-sum twin's logit differs from the
    emulation's on one row in five) moves the logit by a whole ulp.  The band's
    floor is one fp16 ulp of the score; where a logit ulp is worth more than
    that -- for s < 0.25: e.g. s = 0.09, y = -2.3, ulp16(y) = 2^-9, times
    s (1 - s) = 0.082 is 1.6e-4 = 2.6 ulp16(s) -- no implementation of the
    stated arithmetic can be held to the floor.  It holds for every s >= 0.25:
    the cases keep their scores there (checked by a CPU test)."""
    s = score.double()
    return fp16_ulp(logit) * s * (1 - s) <= fp16_ulp(s)


def row_tolerance(emu, twins):
    """tol_row = 4 x the spread of the twins around the emulation + one fp16 ulp
    of the score.  (spread_row, tol_row)."""
    spread = torch.zeros_like(emu)
    for _, t in twins:
        spread = torch.maximum(spread, (t.double() - emu).abs())
    return spread, 4 * spread + fp16_ulp(emu)


def assert_scores_within_band(got, emu, ref64, tol_row, e_row):
    """THE assertion of the GPU tests, on the CPU so that mutants can be fed to
    it: every row within tol_row of the emulation, and no further from float64
    than 3 x the emulation's own error + 2e-3."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), 'non-finite score'
    d_emu, d_64 = (got - emu).abs(), (got - ref64).abs()
    bad = (d_emu > tol_row).nonzero().flatten().tolist()
    assert not bad, (f'rows {bad[:8]} outside tol_row of the fp16 emulation: '
                     f'{d_emu[bad[:8]].tolist()} > {tol_row[bad[:8]].tolist()}')
    bad = (d_64 > 3 * e_row + 2e-3).nonzero().flatten().tolist()
    assert not bad, f'rows {bad[:8]} further from float64 than 3 e_row + 2e-3'


# --------------------------------------------------------------------------
# The committed cases (tests/golden/make_golden_oracle_net.py writes their
# inputs and witness rows into tests/golden/oracle_net_cases.npz)
# --------------------------------------------------------------------------
# name: heads, layers, feed-forward width, seed, scale of the q/k/v weights, further scale of
# the last layer's q/k weights, scale of the head's weights, offset of the head's bias (chosen
# on the CPU, against this reference only, so that the scores spread without saturating, every
# mutant has a witness row, and every row satisfies `logit_rounding_fits`)
CASES = {
    'h4_l2': dict(n_head=4, n_layers=2, ff=64, seed=62, qkv=3.0, qk_last=2.0, head=3.0),
    'h2_l2': dict(n_head=2, n_layers=2, ff=64, seed=47, qkv=3.0, qk_last=1.5, head=3.0,
                  head_bias=3.8),
    'h1_l2': dict(n_head=1, n_layers=2, ff=64, seed=52, qkv=2.0, qk_last=2.0, head=3.0,
                  head_bias=2.4),
    'h4_l1': dict(n_head=4, n_layers=1, ff=64, seed=24, qkv=1.5, head=3.0, head_bias=2.3),
    # the wide feed-forward block: chunk-skip mutants only (first, last, one per wave of the
    # workgroup kernel's hidden split c = w, w + 4, ...), on every eighth row of the inputs
    'h4_l2_ff4096': dict(n_head=4, n_layers=2, ff=4096, seed=25, qkv=3.0, head=3.0, head_bias=2.1,
                         stride=8,
                         only=[('skip_ff_chunk', l, c) for l in (0, 1)
                               for c in (0, 41, 82, 123, 127)]),
}
N_NEEDLE, N_ROUGH = 127, 376
ROUGH0, DEGENERATE0 = N_NEEDLE, N_NEEDLE + N_ROUGH
ROWS = DEGENERATE0 + 8                              # 511: one launch of the workgroup kernel


def case_model(cfg):
    """The seeded TransformerOracle of a case: the default initialisation with
    weights of a trained network's size (biases and LayerNorm parameters that
    are not 0 / 1, so that omitting one shows)."""
    from tracktolearn_amd.oracles.transformer_oracle import TransformerOracle
    state = torch.random.get_rng_state()
    torch.manual_seed(cfg['seed'])
    model = TransformerOracle(381, 1, cfg['n_head'], cfg['n_layers'], 1e-4)
    for layer in model.bert.layers:
        layer.linear1 = torch.nn.Linear(32, cfg['ff'])
        layer.linear2 = torch.nn.Linear(cfg['ff'], 32)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if 'in_proj_weight' in name:
                p.mul_(cfg['qkv'])
            elif name.endswith('bias') or 'norm' in name:
                p.add_(0.2 * torch.randn_like(p))
        # the last layer's queries and keys: how sharply the CLS query picks its keys
        model.bert.layers[-1].self_attn.in_proj_weight[:64].mul_(cfg.get('qk_last', 1.0))
        model.head.weight.mul_(cfg['head'])
        model.head.bias.add_(cfg.get('head_bias', 0.0))
    torch.random.set_rng_state(state)
    return model.eval()


def case_inputs(seed):
    """(ROWS, 127, 3) float32 segment vectors, seeded.  Three families:

    * needles -- row s has ONE segment of norm 2 to 4 at position s (token s + 1) on a
      background (s mod 3) of zero segments, of a smooth walk (~0.1 per segment) or of small
      independent segments;
    * rough -- independent segments of mixed length, randn * rand, up to ~1 long: the rows
      on which single keys matter (every row attends to a different handful of them); the
      second half rounded to values exactly representable in fp16;
    * degenerate -- zero length, constant, near-constant, every segment of norm 2 to 4,
      float32 denormals, values that are denormal in fp16, and two rows of values on and
      next to fp16's rounding ties.
    """
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    unit = lambda d: d / d.norm(dim=-1, keepdim=True)
    x = torch.zeros(ROWS, 127, 3)
    bg = torch.stack([torch.zeros(127, 127, 3),
                      rn(127, 1, 3) * 0.1 + torch.cumsum(rn(127, 127, 3) * 0.05, 1) * 0.3,
                      rn(127, 127, 3) * ru(127, 127, 1) * 0.2], dim=1)      # [s][background]
    bg = bg[torch.arange(127), torch.arange(127) % 3]
    bg[torch.arange(127), torch.arange(127)] = unit(rn(127, 3)) * (2 + 2 * ru(127, 1))
    x[:ROUGH0] = bg
    rough = rn(N_ROUGH, 127, 3) * ru(N_ROUGH, 127, 1)
    rough[N_ROUGH // 2:] = rough[N_ROUGH // 2:].half().float()
    x[ROUGH0:DEGENERATE0] = rough
    d = DEGENERATE0
    x[d] = 0                                                    # a streamline of zero length
    x[d + 1] = torch.tensor([0.3, -0.2, 0.1])                   # constant
    x[d + 2] = torch.tensor([0.3, -0.2, 0.1]) + 1e-4 * rn(127, 3)
    x[d + 3] = unit(rn(127, 3)) * (2 + 2 * ru(127, 1))          # every segment of norm 2 to 4
    x[d + 4] = rn(127, 3) * 1e-40                               # float32 denormals
    x[d + 5] = rn(127, 3) * 3e-6                                # fp16 denormals after rounding
    x[d + 6] = (1 + 2.0 ** -11) * unit(rn(127, 3))              # not representable, near ties
    x[d + 7] = rn(127, 3) * 0.3
    x[d + 7, ::2] += 2.0 ** -12
    return x.float().contiguous()


def case_mutants(cfg):
    """The mutant list of a case, in the order of the fixture's witness table."""
    return list(cfg['only']) if 'only' in cfg else mutants(cfg['n_layers'], cfg['n_head'], cfg['ff'])


def case_rows(cfg):
    """The inputs of a case: all ROWS rows, or every ``stride``-th of them."""
    return case_inputs(cfg['seed'])[::cfg.get('stride', 1)].contiguous()
