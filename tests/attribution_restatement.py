"""Gradient x input attribution restated in fp64, vectorised torch, no GPU: what `drin_token_attribution`,
`drin_rows_dot` and `Model.attribute` are held to.  Every function returns `(A, S)`: the attribution and its cancellation-free
scale `S = sum |x g|` over the same axes - a relative error of `A` alone means nothing where its terms cancel."""
import torch

from oracle import drin_oracle as O

F64 = torch.float64
# the float tensors of the 14-sequence autograd reaches (tests/test_gpu_input_grads.py: FLOAT_INPUTS) ...
FLOAT_INPUTS = {0: "mention_text", 4: "mention_image", 5: "mention_object", 6: "mention_object_score", 7: "entity_text",
                9: "entity_image", 10: "entity_object", 11: "entity_object_score", 12: "miet_similarity", 13: "mtei_similarity"}
# ... and the ones `Model.attribute` returns: (position, dims kept).  The object feature rows enter only cosines: identically 0
ATTRIBUTED = {"mention_text": (0, 2), "mention_image": (4, 2), "mention_object_score": (6, 2), "entity_text": (7, None),
              "entity_image": (9, 2), "entity_object_score": (11, 3), "miet_similarity": (12, 2), "mtei_similarity": (13, 2)}


def kept_tokens(mask: torch.Tensor):
    """`(kept [..., T] bool, cnt [...])` of the entity pooling `x[1:ntok - 1]`, `ntok = sum(mask)` (ghmfc.py:245-249, python slice
    semantics: ntok == 0 gives the stop -1): the tokens `drin_pool_bwd` gives a non-zero share, and how many they are."""
    T = mask.shape[-1]
    stop = mask.to(torch.int64).sum(-1) - 1
    stop = torch.where(stop < 0, stop + T, stop).clamp(0, T)
    t = torch.arange(T, device=mask.device)
    return (t >= 1) & (t < stop.unsqueeze(-1)), (stop - 1).clamp(min=0)


def token_attribution(tokens, mask, grad_pooled, index=None):
    """`drin_token_attribution`: tokens `[P, T, D]` or a table `[E, T, D]` with `index [P]` (clamped into the table), mask alike,
    `grad_pooled [P, D]` -> `A, S [P, T]`."""
    if index is not None:
        index = index.clamp(0, tokens.shape[0] - 1)
        tokens, mask = tokens[index], mask[index]
    kept, cnt = kept_tokens(mask)
    prod = tokens.to(F64) * grad_pooled.to(F64).unsqueeze(-2)
    den = cnt.clamp(min=1).to(F64).unsqueeze(-1)
    zero = torch.zeros((), dtype=F64, device=prod.device)
    return torch.where(kept, prod.sum(-1) / den, zero), torch.where(kept, prod.abs().sum(-1) / den, zero)


def rows_dot(x, g, lead=1):
    """`drin_rows_dot`: everything behind the first `lead` dims is the row."""
    prod = (x.to(F64) * g.to(F64)).reshape(*x.shape[:lead], -1)
    return prod.sum(-1), prod.abs().sum(-1)


def gradient_x_input(inputs, grads):
    """`{field: (A, S)}` of `Model.attribute`'s fields from the batch tensors (the 14-sequence) and their full gradients
    (`{field: tensor}`, the shapes of the inputs): `(x * x.grad).sum(feature axes)`."""
    out = {}
    for field, (i, lead) in ATTRIBUTED.items():
        x, g = inputs[i], grads[field]
        if field == "entity_text":
            lead = 3 if x.dim() == 4 else 2
        if x.dim() == lead:
            prod = x.to(F64) * g.to(F64)
            out[field] = (prod, prod.abs())
        else:
            out[field] = rows_dot(x, g, lead)
    return out


def oracle_input_grads(cfg, sd, batch, G, dtype=F64):
    """Autograd of the oracle on the batch as given (as `oracle_grads` of tests/test_gpu_input_grads.py): `(scores, {field: grad})`."""
    inputs = [t.detach().cpu() for t in batch[:14]]
    for i in FLOAT_INPUTS:
        inputs[i] = inputs[i].to(dtype).requires_grad_(True)
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    scores = O.forward(p, inputs, dtype=dtype, **O.config_kwargs(cfg))
    (scores * G.detach().cpu().to(dtype)).sum().backward()
    return scores.detach(), inputs, {FLOAT_INPUTS[i]: inputs[i].grad for i in FLOAT_INPUTS}


def oracle_attribution(cfg, sd, batch, G, dtype=F64):
    """`(scores, {field: (A, S)})`: gradient x input of `sum(G * scores)` by the oracle's autograd."""
    scores, inputs, grads = oracle_input_grads(cfg, sd, batch, G, dtype)
    return scores, gradient_x_input([t.detach() if torch.is_tensor(t) else t for t in inputs], grads)


def one_hot(candidate, N):
    G = torch.zeros(candidate.shape[0], N, dtype=F64)
    G[torch.arange(candidate.shape[0]), candidate.cpu()] = 1.0
    return G
