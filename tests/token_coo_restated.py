"""The semantics of isg_token_coo restated as plain Python loops over ids (include/isg.h).  Every result is an integer, so the GPU
tests compare with it exactly.  Not a test module: tests/test_token_coo_cpu.py holds it to what the reference's three functions
return on strings (tests/golden/g11_token_coo.pt), tests/test_gpu_token_coo.py holds the kernel to it."""
import torch

TOKENS_MAX = 128
HIST = TOKENS_MAX + 1
TOTALS = 16 + 4 * HIST


def _f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


def restate_table(names, node_mask, ptr, pred, label, ans_sg, qtok=None, ttok=None, tkeep=None, threshold=0.0):
    """int32 [B, 8].  names int64 [N], node_mask fp32 [N] or [N, 1], ptr [B + 1], pred / label [B], ans_sg [A], qtok [B, T],
    ttok / tkeep [B, T2] (host tensors or lists)."""
    names = [int(v) for v in torch.as_tensor(names).reshape(-1).tolist()]
    mask = torch.as_tensor(node_mask, dtype=torch.float32).reshape(-1).tolist()
    ptr = [int(v) for v in torch.as_tensor(ptr).tolist()]
    pred, label = torch.as_tensor(pred).tolist(), torch.as_tensor(label).tolist()
    ans_sg = torch.as_tensor(ans_sg).tolist()
    thr = _f32(threshold)                                    # the C ABI takes a float
    B = len(pred)
    rows = []
    for g in range(B):
        nodes = range(ptr[g], ptr[g + 1])
        in_graph = {names[n] for n in nodes}
        in_kept = {names[n] for n in nodes if mask[n] > thr}         # a NaN compares false
        graph = lambda v: int(v >= 0 and v in in_graph)
        kept = lambda v: int(v >= 0 and v in in_kept)
        answer = lambda cls: ans_sg[cls] if 0 <= cls < len(ans_sg) else -1
        p, l = answer(pred[g]), answer(label[g])
        words = [] if qtok is None else [int(v) for v in qtok[g]]
        text = [] if ttok is None else [int(v) for v, k in zip(ttok[g], torch.as_tensor(tkeep[g], dtype=torch.float32).tolist())
                                        if k == 1.0]
        rows.append([int(pred[g] == label[g]), graph(p), graph(l), kept(p), sum(graph(v) for v in words), sum(kept(v) for v in words),
                     sum(graph(v) for v in text), sum(kept(v) for v in text)])
    return torch.tensor(rows, dtype=torch.int32).view(B, 8)


def add_totals(totals, table, qflags=None):
    """`totals` (a list of TOTALS ints, or None for zeros) with the rows of `table` added: a new list."""
    t = [0] * TOTALS if totals is None else [int(v) for v in totals]
    for g, row in enumerate(torch.as_tensor(table).tolist()):
        correct, pred_in, label_in, ans_kept, words, words_kept, text, text_kept = row
        color = 0 if qflags is None else int(qflags[g]) & 1
        t[0] += 1
        t[1] += correct
        t[2] += pred_in
        t[3] += correct & pred_in
        ans_valid = correct and label_in and not color
        t[4] += int(bool(ans_valid))
        t[5] += int(bool(ans_valid and ans_kept))
        for first, hist, m, hits in ((6, 16, words, words_kept), (9, 16 + 2 * HIST, text, text_kept)):
            if correct and m > 0:
                t[first] += 1
                t[first + 1] += m
                t[first + 2] += hits
                t[hist + m] += 1
                t[hist + HIST + m] += hits
    return t
