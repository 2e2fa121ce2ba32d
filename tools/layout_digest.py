"""One ``case sha256`` line per arena / bucket layout case, read from a CPU ``TrainEngine``: run on
two trees and diff the output to show that a change kept where every parameter lives and which
arena ranges are exchanged.  Each line hashes offsets, numel, train_hi, acc_hi, lazy, ln_order, the
LayerNorm offsets, frozen, the bucket bounds and reduced ranges, bucket_after, ln_done_at,
temb_bucket, reduced_numel and sq_tiles as canonical JSON (sorted keys, plain ints).  The facts are
read under whichever names the tree has (``eng.layout`` / ``eng.bucketing``, or the engine's own
attributes before those existed).  Cases: three models x temb_rows x timestep_embedding x
weight_ema x force_segments x bucket_blocks x embed_bucket.
python tools/layout_digest.py [case-substring ...]"""
import hashlib, itertools, json, os, sys
from collections.abc import Mapping
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddim_cold_amd import build_model
from ddim_cold_amd.models import DiffusionVisionTransformer
from ddim_cold_amd.train.engine import EngineConfig, TrainEngine

MODELS = {
    "vit_tiny": lambda **kw: build_model("vit_tiny", **kw),
    "vit_small_200": lambda **kw: build_model("vit_small_200", **kw),
    "16x16 depth 3": lambda **kw: DiffusionVisionTransformer(img_size=[16, 16], patch_size=4, embed_dim=32, depth=3,
                                                             num_heads=2, **kw),
}
TEMB_ROWS = (7, None)
TIMESTEP_EMBEDDING = ("learned", "sinusoidal")
WEIGHT_EMA = (0.0, 0.99)
FORCE_SEGMENTS = (True, False)
BUCKET_BLOCKS = (1, 2, 3, 4, 7, 1 << 16)
EMBED_BUCKET = (True, False)


def plain(x):
    """Tuples, sets and int-keyed mappings as JSON lists in a fixed order."""
    if isinstance(x, Mapping):
        return [[plain(k), plain(v)] for k, v in sorted(x.items())]
    if isinstance(x, (set, frozenset)):
        return sorted(x)
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x if x is None or isinstance(x, str) else int(x)


def facts(eng) -> dict:
    lay, bk = getattr(eng, "layout", eng), getattr(eng, "bucketing", eng)
    new = bk is not eng
    return dict(
        offsets=lay.offsets, numel=lay.numel, train_hi=lay.train_hi, acc_hi=lay.acc_hi, lazy=eng.lazy,
        ln_order=lay.ln_order, ln_offs=lay.ln_offs if new else eng._ln_offs(), frozen=lay.frozen,
        bounds=bk.bounds if new else eng.buckets, ranges=bk.ranges if new else eng.bucket_ranges,
        bucket_after=bk.bucket_after, ln_done_at=bk.ln_done_at, temb_bucket=bk.temb_bucket,
        reduced_numel=eng.reduced_numel(), sq_tiles=lay.sq_tiles if new else eng._sq_tiles)


def main(want):
    for name, rows, temb, ema, seg in itertools.product(MODELS, TEMB_ROWS, TIMESTEP_EMBEDDING, WEIGHT_EMA,
                                                        FORCE_SEGMENTS):
        head = f"{name} temb_rows={rows} {temb} weight_ema={ema} force_segments={seg}"
        if want and not any(w in head for w in want):
            continue
        # one engine per arena layout; the bucket layouts are its set_comm_layout() results
        eng = TrainEngine(MODELS[name](timestep_embedding=temb),
                          EngineConfig(temb_rows=rows, weight_ema=ema, force_segments=seg, use_graph=False), device="cpu")
        for bb, eb in itertools.product(BUCKET_BLOCKS, EMBED_BUCKET):
            eng.set_comm_layout(bb, eb)
            text = json.dumps({k: plain(v) for k, v in facts(eng).items()}, sort_keys=True, separators=(",", ":"))
            print(f"{head} bucket_blocks={bb} embed_bucket={eb} {hashlib.sha256(text.encode()).hexdigest()[:32]}",
                  flush=True)
        eng.detach()


if __name__ == "__main__":
    main(sys.argv[1:])
