"""Model factory with the reference's entry point: ``build_model(args, cfg)`` (ISubGVQA/models/build.py:4-27).

The flags that select the hot path's variants are read off the argparse namespace by name and handed to the model as
keywords; I-MLE style sampling is always on, as in the reference.  Three flags are this project's own and optional:
``sample_ratio`` / ``sample_k_min`` (a node budget per graph with ``sample_k`` as its cap), read by ISubGVQA with
``getattr(args, "sample_ratio", None)`` / ``getattr(args, "sample_k_min", 1)`` -- a reference Namespace has neither.  A third,
``attn_dropout`` (dropout on the GATv2 layers' attention weights in training), is read the same way with 0.0."""
from .isubgvqa import ISubGVQA

# namespace attribute -> ISubGVQA keyword (identical names; listed so that a missing flag fails here, by name)
_FORWARDED = ("use_masking", "use_instruction", "use_mgat", "mgat_masks", "use_topk", "interpretable_mode",
              "concat_instr", "embed_cat")


def build_model(args, cfg=None):
    missing = [name for name in _FORWARDED if not hasattr(args, name)]
    if missing:
        raise AttributeError(f"build_model: args lacks {missing} (see ISubGVQA/utils/arg_parser.py)")
    kwargs = {name: getattr(args, name) for name in _FORWARDED}
    net = ISubGVQA(args, use_imle=True, **kwargs)
    return net.to(device=args.device)
