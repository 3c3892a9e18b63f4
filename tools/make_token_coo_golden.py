#!/usr/bin/env python3
"""Writes tests/golden/g11_token_coo.pt: a small vocabulary and a few hundred scoring cases as STRINGS, each with what the
reference's three functions (ISubGVQA/utils/token_coo_fns.py, imported at run time from a checkout of the reference) return for
it, and the five figures run_token_coo.py:181-185 prints over several lists of cases (its np.mean / np.nanmean expressions, on the
lists its loop at :145-173 builds).  tests/test_token_coo_cpu.py reproduces all of it from the strings through
explain.TokenTables, the restatement of tests/token_coo_restated.py and explain.CooReport.

    python3 tools/make_token_coo_golden.py --reference /path/to/reference [--out tests/golden/g11_token_coo.pt]
"""
import argparse
import importlib.util
import os
import random
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

OBJ1 = ["cat", "dog", "man", "woman", "table", "chair", "tree", "car", "bus", "shirt", "hat", "ball", "plate", "window", "sky",
        "grass"]
OBJ2 = ["traffic light", "tennis racket", "fire hydrant", "teddy bear"]
ATTR = ["red", "blue", "small", "large", "wooden", "left", "right"]
FILLER = ["is", "the", "there", "a", "what", "color", "near", "or", "it", "sunny", "today", "big", "on", "who", "holding", "to", "of"]
ANSWERS = OBJ1 + OBJ2 + ["yes", "no", "left", "right", "red", "blue", "bottom"]
SPECIALS = ["<unk>", "<pad>", "<sos>", "<eos>", "<self>"]
KINDS = ["ans_hit", "ans_miss", "ans_color", "ans_absent", "qst_partial_repeat", "qst_nan", "text_nan", "text_some", "multiword",
         "double_space", "nan_mask", "at_threshold", "empty_graph"]
PER_KIND = 18


def vocabulary():
    stoi = {t: i for i, t in enumerate(SPECIALS + OBJ1 + OBJ2 + ATTR)}
    clip_itos = ["<|startoftext|>", "<|endoftext|>"] + [w + "</w>" for w in OBJ1 + ATTR + FILLER]
    clip_itos += ["traffic</w>", "light</w>", "tennis</w>", "racket</w>", "teddy</w>", "bear</w>", "ca", "t</w>", "?</w>"]
    return stoi, clip_itos


def clip_ids(question, clip_itos, length=14):
    """BOS, the question's words that are whole CLIP tokens of this toy vocabulary (the rest as the two pieces `ca` `t</w>`), a
    question mark, EOS, padded with EOS -- the layout of a CLIP tokenisation; no tokenizer is involved."""
    where = {t: i for i, t in enumerate(clip_itos)}
    ids = [0]
    for w in question.split("?")[0].lower().split(" "):
        ids += [where[w + "</w>"]] if w + "</w>" in where else [where["ca"], where["t</w>"]]
    ids += [where["?</w>"], 1]
    return (ids + [1] * length)[:length]


def build(rng, kind):
    thr = 0.0
    n = 0 if kind == "empty_graph" else rng.randint(2, 9)
    objects = [rng.choice(OBJ1) for _ in range(n)]
    mask = [rng.choice((0.0, 0.0, 1.0, 1.0, 0.25, -1.0)) for _ in range(n)]
    j = rng.randrange(n) if n else 0
    a = objects[j] if n else "cat"
    absent = [o for o in OBJ1 if o not in objects]
    label = answer = rng.choice(ANSWERS)
    question = rng.choice([f"Is there a {a} near the {rng.choice(OBJ1)}?", f"Is the {a} {rng.choice(ATTR)}?",
                           f"What is near the {rng.choice(OBJ1)}?", f"Who is holding the {a}?"])
    keep = None
    drop_all = lambda name: [0.0 if o == name else m for o, m in zip(objects, mask)]
    if kind == "ans_hit":
        mask[j] = 1.0
        label = answer = a
    elif kind == "ans_miss":
        mask = drop_all(a)
        label = answer = a
    elif kind == "ans_color":
        label = answer = a
        question = rng.choice([f"What color is the {a}?", f"Is the {a} the same color?", f"Which colors is the {a}?"])
    elif kind == "ans_absent":
        label = answer = rng.choice(absent + ["yes", "no", "bottom"])
    elif kind == "qst_partial_repeat":
        b = rng.choice([o for o in objects if o != a] or absent)
        if b not in objects:
            objects.append(b)
            mask.append(0.0)
        mask = drop_all(b)
        mask[j] = 1.0
        question = f"Is the {a} near the {b} or the {a}?"
    elif kind == "qst_nan":
        question = rng.choice(["Is it sunny today?", f"Is there a {absent[0]} on the {absent[1]}?", "What is it?"])
    elif kind == "text_nan":
        keep = "none" if rng.random() < 0.5 else "fillers"
    elif kind == "text_some":
        question = f"Is the {a} near the {rng.choice(OBJ1)}?"
        keep = "objects"
    elif kind == "multiword":
        mw = rng.choice(OBJ2)
        objects.insert(j, mw)
        mask.insert(j, rng.choice((1.0, 0.0)))
        label = answer = mw
        question = f"Is the {mw} near the {a}?"
    elif kind == "double_space":
        question = rng.choice([f"Is the  {a} big?", f"Is  there a {a}  near it?", f" What is near the {a}?"])
    elif kind == "nan_mask":
        mask[j] = NAN
        label = answer = a
        question = f"Is the {a} big?"
    elif kind == "at_threshold":
        thr = rng.choice((0.0, 0.5, 0.25))
        mask = [thr if o == a else m for o, m in zip(objects, mask)]
        label = answer = a
        question = f"Is the {a} big?"
    if not kind.startswith("ans_") and rng.random() < 0.25:
        answer = rng.choice([x for x in ANSWERS if x != label])
    return dict(kind=kind, objects=objects, mask=mask, threshold=thr, question=question, answer=answer, label=label, keep=keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (holds ISubGVQA/utils/token_coo_fns.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g11_token_coo.pt"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("token_coo_fns", os.path.join(args.reference, "ISubGVQA", "utils", "token_coo_fns.py"))
    fns = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fns)
    rng = random.Random(11)
    stoi, clip_itos = vocabulary()
    cases = [build(rng, kind) for _ in range(PER_KIND) for kind in KINDS]
    strip = [t.replace("</w>", "") for t in clip_itos]
    for c in cases:
        ids = clip_ids(c["question"], clip_itos)
        how = c.pop("keep") or rng.choice(("random", "random", "all"))
        named = lambda i: strip[i] in c["objects"]
        tkeep = [{"none": 0.0, "all": 1.0, "random": rng.choice((1.0, 0.0, 0.999, 1.0)), "fillers": 0.0 if named(i) else 1.0,
                  "objects": 1.0 if named(i) or rng.random() < 0.3 else 0.0}[how] for i in ids]
        if c["kind"] == "text_nan" and how == "none":
            tkeep[1] = NAN                                   # a NaN is not 1.0
        c["input_ids"], c["tkeep"] = ids, tkeep
        # run_token_coo.py:82-88 on a [T] token mask
        keep_t = torch.tensor(tkeep, dtype=torch.float32)
        text_expl = [clip_itos[int(t)].replace("</w>", "") for i, t in enumerate(ids) if keep_t[i] == 1.0]
        mask = torch.tensor(c["mask"], dtype=torch.float32).view(-1, 1)              # the forward's imle_mask
        c["ans"] = tuple(fns.compute_ans_token_cooccurrence(mask=mask, ans_token=c["answer"], label_gt=c["label"], objects=c["objects"],
                                                            qst_tokens=c["question"], threshold=c["threshold"]))
        c["qst"] = tuple(fns.compute_qst_token_cooccurrence(mask=mask, objects=c["objects"], qst_tokens=c["question"],
                                                            threshold=c["threshold"]))
        c["text"] = float(fns.compute_text_expl_token_cooccurrence(mask=mask, objects=c["objects"], text_expl_tokens=text_expl,
                                                                   qst_tokens=c["question"], threshold=c["threshold"]))
    # the loop of run_token_coo.py:145-173 and the prints of :181-185 over lists of cases
    every = list(range(len(cases)))
    lists = {"all": (every, True), "first_60": (every[:60], True), "every_third": (every[::3], True), "no_text": (every, False),
             "wrong_only": ([i for i in every if cases[i]["answer"] != cases[i]["label"]], True), "none": ([], True)}
    aggregates = {}
    for name, (idx, with_text) in lists.items():
        accuracy, accuracy_at, ans_list, qst_list, text_list = [], [], [], [], []
        for i in idx:
            c = cases[i]
            accuracy.append(float(c["answer"] == c["label"]))
            if c["answer"] in c["objects"]:
                accuracy_at.append(float(c["answer"] == c["label"]))
            if c["answer"] == c["label"]:
                if with_text:
                    text_list.append(c["text"])
                ans_list.append(c["ans"])
                qst_list.append(c["qst"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            aggregates[name] = {"cases": idx, "with_text": with_text,
                                "printed": {"Accuracy": float(np.mean(accuracy)), "Accuracy AT": float(np.mean(accuracy_at)),
                                            "Ans. Tok. Coo": float(np.nanmean(ans_list)), "Qst. Tok. Coo": float(np.nanmean(qst_list)),
                                            "Qst. Text Tok. Coo": float(np.nanmean(text_list))}}
    # one float32 tensor for all masks / token masks (a tensor per case would cost more than the case)
    masks = torch.tensor([m for c in cases for m in c["mask"]], dtype=torch.float32)
    tkeeps = torch.tensor([m for c in cases for m in c["tkeep"]], dtype=torch.float32)
    for c in cases:
        c["mask"], c["tkeep"] = len(c["mask"]), len(c["tkeep"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    torch.save({"stoi": stoi, "answers": ANSWERS, "clip_itos": clip_itos, "cases": cases, "masks": masks, "tkeeps": tkeeps,
                "aggregates": aggregates}, args.out)
    print(f"{args.out}: {len(cases)} cases, {os.path.getsize(args.out)} bytes")
    for name, agg in aggregates.items():
        print(name, len(agg["cases"]), agg["printed"])


if __name__ == "__main__":
    main()
