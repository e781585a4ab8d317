"""Path-pinned inputs for the two device forms of EfficientNMS (csrc/nms.hip) and a coarse CPU model of which device paths an
input reaches in the multi-workgroup form (yv_efficient_nms_ws).

The model restates the conditions of the launcher and of en2_front_kernel on the CPU:

    seg_list / atomic_list       A*nc <= 45056: one 4096-entry list region per filter chunk, no counter, no memset launch
    tail / classes+merge         nc <= 8: one launch for the light classes and the merge; else a (nc, B) grid and a merge launch
    cc_lds / cc_global           per-class counters staged in LDS (nc <= 2048) or added straight to the workspace
    filter_vec                   a filter workgroup takes the 16-byte loads (aligned image base, chunk inside the image)
    filter_tail_chunk            the image's last chunk is short: 4-byte loads with a bound
    filter_unaligned             an image's score block does not start on 16 bytes: 4-byte loads for all of its chunks
    head16 / head44 / head_none  candidates of an image: <= 16384 (16 keys per thread), <= list capacity (44), more (no head)
    head_all_equal               more candidates than the head holds and not one bit differs between their keys
    general                      the head cannot finish the image: select (if needed), per-class NMS, merge
    seg_compact_inplace          general, segmented list, no select: the list is made contiguous in place ...
    seg_compact_multichunk       ... and candidates of a later chunk really move
    select_reg / select_bitserial  more candidates than pre_topk: radix select on register keys (A*nc <= 45056), else bit-serial
    cut_ties_partial             only some of the candidates that tie on the cut key belong to the selected set
    heavy                        general, and a class of the selected set has more than 1024 candidates (done by en2_front_kernel)

`general` is claimed only where it is certain: the image has more candidates than the list holds; or more than the head
holds (min(pre_topk, 512)) while the whole scan keeps fewer than max_out (any prefix then keeps fewer too); or all candidate
scores are equal and outnumber the head.  The head's window arithmetic (which prefix of 160..320 candidates it takes and
whether max_out boxes are kept inside it) is NOT modelled: an image outside the three rules reports neither `general` nor
any of the paths behind it.
"""
import functools

import torch

from oracle import boxes as ob

FILTER_CHUNK = 4096          # EN2_FT * EN2_FPT
SEG_SCORES = 45056           # EN2_HRW * EN_THREADS = EN2_SEGS * FILTER_CHUNK
HEAD = 512                   # EN2_HEAD
HEAD16 = 16384               # EN2_HR * EN_THREADS
CC_LDS = 2048                # EN2_CC_LDS
TAIL_NC = 8                  # EN2_TAIL_NC
LIGHT = 1024                 # classes up to this many selected candidates go to the 256-thread tier

PATHS = ("seg_list", "atomic_list", "tail", "classes+merge", "cc_lds", "cc_global", "filter_vec", "filter_tail_chunk",
         "filter_unaligned", "head16", "head44", "head_none", "head_all_equal", "general", "seg_compact_inplace",
         "seg_compact_multichunk", "select_reg", "select_bitserial", "cut_ties_partial", "heavy")


def list_capacity(A, nc, topk):
    total = A * nc
    c = (total + FILTER_CHUNK - 1) // FILTER_CHUNK * FILTER_CHUNK if total <= SEG_SCORES else SEG_SCORES
    return (max(c, topk) + 63) & ~63


def paths(boxes, scores, thr=0.25, iou=0.65, max_out=100, topk=4096):
    """The set of path names (see the module docstring) that yv_efficient_nms_ws takes for this input."""
    B, A, nc = scores.shape
    total = A * nc
    lcap = list_capacity(A, nc, topk)
    seg = total <= SEG_SCORES
    out = {"seg_list" if seg else "atomic_list", "tail" if nc <= TAIL_NC else "classes+merge",
           "cc_lds" if nc <= CC_LDS else "cc_global"}
    for b in range(B):
        aligned = (b * total * 4) % 16 == 0           # (the tensor itself is at least 16-byte aligned)
        if not aligned:
            out.add("filter_unaligned")
        if aligned and total >= FILTER_CHUNK:
            out.add("filter_vec")
        if total % FILTER_CHUNK:
            out.add("filter_tail_chunk")
    kept = None
    for b in range(B):
        flat = scores[b].reshape(-1).float()
        cand = torch.nonzero(flat > thr).reshape(-1)
        cnt = int(cand.numel())
        out.add("head16" if cnt <= HEAD16 else "head44" if cnt <= lcap else "head_none")
        head = min(topk, HEAD)
        all_equal = cnt > head and cnt <= lcap and bool((flat[cand] == flat[cand[0]]).all())
        if all_equal:
            out.add("head_all_equal")
        general = cnt > lcap or all_equal
        if not general and cnt > head:
            if kept is None:
                kept = ob.efficient_nms(boxes, scores, thr, iou, max_out, topk)[0].reshape(-1)
            general = int(kept[b]) < max_out
        if not general:
            continue
        out.add("general")
        sel = cand
        if cnt > topk:
            out.add("select_reg" if (total + 1023) // 1024 <= 44 else "select_bitserial")
            order = torch.sort(flat[cand], descending=True, stable=True).indices
            sel = cand[order][:topk]
            cut = flat[sel[-1]]
            if int((flat[cand] == cut).sum()) > int((flat[sel] == cut).sum()):
                out.add("cut_ties_partial")
        elif seg:
            out.add("seg_compact_inplace")
            if bool((cand >= FILTER_CHUNK).any()):
                out.add("seg_compact_multichunk")
        if int(torch.bincount(sel % nc, minlength=nc).max()) > LIGHT:
            out.add("heavy")
    return out


def clustered(B, A, nc, n_clusters, seed=0, power=1.0):
    """Clusters of near-identical boxes (heavy suppression: the scan walks many tiles before max_out boxes are kept)."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(B, n_clusters, 2, generator=g) * 560 + 40
    pick = torch.randint(0, n_clusters, (B, A), generator=g)
    c = torch.gather(centres, 1, pick[..., None].expand(B, A, 2)) + torch.randn(B, A, 2, generator=g) * 3
    wh = 60 + torch.randn(B, A, 2, generator=g).abs() * 6
    boxes = torch.cat([c - wh / 2, c + wh / 2], -1).contiguous()
    scores = torch.rand(B, A, nc, generator=g) ** power
    return boxes, scores


def _identical_many_classes():
    g = torch.Generator().manual_seed(5)
    B, A, nc = 2, 4, 2049
    boxes = torch.tensor([100.0, 100.0, 180.0, 190.0]).repeat(B, A, 1).contiguous()
    scores = torch.zeros(B, A, nc)
    live = list(range(299)) + [2048]
    scores[:, :, live] = torch.rand(B, A, len(live), generator=g) * 0.7 + 0.3
    return boxes, scores


def _equal_scores():
    boxes, scores = clustered(1, 1200, 2, 4, seed=9)
    return boxes, torch.full_like(scores, 0.5)


# name -> (input builder, keyword arguments of efficient_nms, paths the case must reach)
CASES = {
    "one_class_select": (lambda: clustered(2, 6000, 1, 12, seed=1), {},
                         {"general", "select_reg", "heavy", "tail", "seg_list", "filter_vec", "filter_tail_chunk", "cc_lds"}),
    "three_classes_select": (lambda: clustered(1, 3000, 3, 12, seed=2), {}, {"general", "select_reg", "heavy"}),
    "atomic_list_head44": (lambda: clustered(1, 4000, 12, 3, seed=3), {},
                           {"head44", "general", "select_bitserial", "atomic_list", "classes+merge"}),
    "atomic_list_no_head": (lambda: clustered(1, 4000, 12, 3, seed=3), {"thr": 0.01},
                            {"head_none", "general", "select_bitserial"}),
    "global_counters": (_identical_many_classes, {"max_out": 600},
                        {"cc_global", "general", "seg_compact_inplace", "seg_compact_multichunk", "classes+merge"}),
    "global_counters_select": (_identical_many_classes, {"max_out": 600, "topk": 1000},
                               {"cc_global", "general", "select_reg"}),
    "unaligned_images": (lambda: clustered(3, 501, 5, 6, seed=7), {},
                         {"filter_unaligned", "general", "seg_compact_inplace", "head16"}),
    "multichunk_compaction": (lambda: clustered(2, 2500, 4, 8, seed=8), {"thr": 0.7},
                              {"general", "seg_compact_inplace", "seg_compact_multichunk", "tail"}),
    "equal_scores": (_equal_scores, {"topk": 1000}, {"head_all_equal", "general", "select_reg", "cut_ties_partial"}),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def case_expected(name):
    """oracle/boxes.py on the case: computed once, shared by the tests, never modified."""
    boxes, scores = case_inputs(name)
    kw = CASES[name][1]
    return ob.efficient_nms(boxes, scores, kw.get("thr", 0.25), kw.get("iou", 0.65), kw.get("max_out", 100), kw.get("topk", 4096))


@functools.lru_cache(maxsize=None)
def case_paths(name):
    boxes, scores = case_inputs(name)
    return frozenset(paths(boxes, scores, **CASES[name][1]))
