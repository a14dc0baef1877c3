"""Plain-torch, dtype-generic, differentiable restatement of the keypoint losses (test infrastructure).

The heatmap and associative-embedding terms of ``ClassMultiLossFactory`` (``Utils/loss.py:641-665``) with
``HeatmapLoss`` (``:17-27``) and ``AELoss`` (``:37-98``); in fp32 the same torch ops as the reference, in the same
order. Runs in any dtype on any device (those of the predictions). ``tools/gen_golden_kp_loss.py`` checks it against
the reference in fp64.

Where it departs from the reference as shipped: an image with no person or with one gives zeros of the predictions'
dtype on their device (``_make_input`` calls ``.cuda()`` and returns fp32, ``:29-34, 60-65``); a visible entry whose
index lies outside the tag planes is skipped, as the kernels skip it (the reference raises ``IndexError``); the
visible tags of a person are read with one index op in place of one per joint plus ``torch.stack`` (the same values in
the same order).
"""
import numpy as np
import torch

OPTIONS = dict(NUM_JOINTS=17, WITH_HEATMAPS_LOSS=(True, True), HEATMAPS_LOSS_FACTOR=(1.0, 1.0),
               WITH_AE_LOSS=(False, False), AE_LOSS_TYPE="exp", PUSH_LOSS_FACTOR=(0.001, 0.001),
               PULL_LOSS_FACTOR=(0.001, 0.001))


def heatmap_loss(pred, gt, mask):
    """HeatmapLoss.forward (:22-27): [B]."""
    assert pred.size() == gt.size()
    loss = ((pred - gt) ** 2) * mask[:, None, :, :].expand_as(pred)
    return loss.mean(dim=3).mean(dim=2).mean(dim=1)


def single_tag_loss(pred_tag, joints, kind):
    """AELoss.singleTagLoss (:42-85): ``pred_tag`` [T, 1], ``joints`` an integer array [P, J, 2]; (push, pull)."""
    T = pred_tag.shape[0]
    zero = pred_tag.new_zeros(1).sum()
    tags = []
    pull = 0
    for person in joints:
        ids = [int(j[0]) for j in person if j[1] > 0 and 0 <= j[0] < T]
        if len(ids) == 0:
            continue
        tmp = pred_tag[torch.as_tensor(ids, device=pred_tag.device)]
        tags.append(torch.mean(tmp, dim=0))
        pull = pull + torch.mean((tmp - tags[-1].expand_as(tmp)) ** 2)
    num_tags = len(tags)
    if num_tags == 0:
        return zero, zero
    if num_tags == 1:
        return zero, pull / num_tags
    tags = torch.stack(tags)
    A = tags.expand(num_tags, num_tags)
    diff = A - A.permute(1, 0)
    if kind == "exp":
        push = torch.sum(torch.exp(-torch.pow(diff, 2))) - num_tags
    elif kind == "max":
        push = torch.clamp(1 - torch.abs(diff), min=0).sum() - num_tags
    else:
        raise ValueError("Unkown ae loss type")
    return push / ((num_tags - 1) * num_tags) * 0.5, pull / num_tags


def ae_loss(tags, joints, kind):
    """AELoss.forward (:87-98): ``tags`` [B, T, 1]; (pushes [B], pulls [B])."""
    joints = np.asarray(joints.cpu() if isinstance(joints, torch.Tensor) else joints)
    pushes, pulls = zip(*(single_tag_loss(tags[i], joints[i], kind) for i in range(tags.size(0))))
    return torch.stack(pushes), torch.stack(pulls)


def keypoint_loss(preds, heatmaps_gt, masks, tag_targets, options=None):
    """(total, terms [3] = heatmap, ae, total, parts [S, 3] = per stage heatmap, push, pull with the factors) as
    ClassMultiLossFactory.forward:639-665 adds them; the labels and masks are cast to the predictions' dtype."""
    opt = dict(OPTIONS, **(options or {}))
    J = opt["NUM_JOINTS"]
    dt, dev = preds[0].dtype, preds[0].device
    zero = torch.zeros((), dtype=dt, device=dev)
    heat, ae, parts = zero, zero, []
    for idx in range(len(preds)):
        h = push = pull = zero
        if opt["WITH_HEATMAPS_LOSS"] and opt["WITH_HEATMAPS_LOSS"][idx]:
            loss = heatmap_loss(preds[idx][:, :J], heatmaps_gt[idx].to(device=dev, dtype=dt),
                                masks[idx].to(device=dev, dtype=dt))
            h = (loss * opt["HEATMAPS_LOSS_FACTOR"][idx]).mean()
            heat = heat + h
        if opt["WITH_AE_LOSS"] and opt["WITH_AE_LOSS"][idx]:
            tags_pred = preds[idx][:, J:]
            tags_pred = tags_pred.contiguous().view(tags_pred.size(0), -1, 1)
            pushes, pulls = ae_loss(tags_pred, tag_targets[idx], opt["AE_LOSS_TYPE"])
            push = (pushes * opt["PUSH_LOSS_FACTOR"][idx]).mean()
            pull = (pulls * opt["PULL_LOSS_FACTOR"][idx]).mean()
            ae = ae + (push + pull)
        parts.append(torch.stack([h.detach(), push.detach(), pull.detach()]))
    total = heat + ae
    return total, torch.stack([heat.detach(), ae.detach(), total.detach()]), torch.stack(parts)


def run(arrays, options, dtype=torch.float64, device="cpu", scale=1.0):
    """Forward + backward of ``scale * total`` from numpy inputs (``pred<s>``, ``gt<s>``, ``mask<s>``, ``tag<s>``):
    {"terms", "parts", "g_pred<s>"} as float64 arrays."""
    S = 0
    while f"pred{S}" in arrays:
        S += 1
    get = lambda k, s: torch.as_tensor(np.asarray(arrays[f"{k}{s}"])).to(device) if f"{k}{s}" in arrays else None
    preds = [get("pred", s).to(dtype).requires_grad_(True) for s in range(S)]
    tags = [None if f"tag{s}" not in arrays else np.asarray(arrays[f"tag{s}"]) for s in range(S)]
    total, terms, parts = keypoint_loss(preds, [get("gt", s) for s in range(S)], [get("mask", s) for s in range(S)],
                                        tags, options)
    if total.requires_grad:
        (total * scale).backward()
    out = {"terms": terms.cpu().double().numpy(), "parts": parts.cpu().double().numpy()}
    for s, p in enumerate(preds):
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        out[f"g_pred{s}"] = g.detach().cpu().double().numpy()
    return out


def person_means(arrays, s, J):
    """fp64 reference tags m_p of every image of stage ``s``: a list over images of the means of its persons."""
    pred, tag = np.asarray(arrays[f"pred{s}"], np.float64), np.asarray(arrays[f"tag{s}"])
    out = []
    for b in range(pred.shape[0]):
        t = pred[b, J:].reshape(-1)
        ms = []
        for person in tag[b]:
            ids = [int(j[0]) for j in person if j[1] > 0 and 0 <= j[0] < t.size]
            if ids:
                ms.append(t[ids].mean())
        out.append(np.asarray(ms))
    return out


def max_kinks_clear(arrays, s, J, margin=1e-3):
    """True when no two person means of an image are equal or within ``margin`` of distance 1: the clamp and the
    absolute value of the 'max' form then take the same branch in every precision."""
    for ms in person_means(arrays, s, J):
        d = np.abs(ms[:, None] - ms[None, :])[~np.eye(len(ms), dtype=bool)]
        if d.size and (np.any(d == 0) or np.any(np.abs(d - 1) < margin)):
            return False
    return True
