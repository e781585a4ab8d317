"""The grouped Detect head on the CPU: the launch list with ConvGroup entries (engines.detect_launches(grouped_head=True)) and the
partition yv_conv2d_group makes of a group (yvhip.conv2d_group_plan, host only - the function the launch itself uses)."""
import collections

import pytest

import yvhip
from yvhip import engines
from yvhip.engines import C2fFused, Conv, ConvGroup, Pool, Stem, detect_launches
from test_gpu_conv_routes import Options as RouteOptions          # (importing the module launches nothing)

LISTS = [(scale, nc, tail) for scale in "nsm" for nc in (5, 80) for tail in (True, False)]


def flat(entries):
    return [c for e in entries for c in (e.convs if type(e) is ConvGroup else (e,))]


def writes(e):
    """(buffer, first channel, end channel or None = all) an entry writes."""
    if type(e) is Conv:
        return [(e.out, e.out_off, e.out_off + e.cout)]
    if type(e) is Pool:
        return [(e.buf, e.c, 4 * e.c)]
    return [(e.out, 0, None)]


def reads(c: Conv):
    r = [(b, off, off + ch) for b, off, ch, _ in c.srcs]
    if c.res_off is not None:
        r.append((c.out, c.res_off, c.res_off + c.cout))
    return r


def overlap(a, b):
    return a[0] == b[0] and (a[2] is None or b[2] is None or (a[1] < b[2] and b[1] < a[2]))


@pytest.mark.parametrize("scale,nc,tail", LISTS)
def test_grouped_list_holds_the_default_lists_entries(scale, nc, tail):
    default = detect_launches(scale, nc, True, tail)
    grouped = detect_launches(scale, nc, True, tail, True)
    groups = [e for e in grouped if type(e) is ConvGroup]
    n_head = 15 if tail else 9
    assert not any(type(e) is ConvGroup for e in default)
    assert len(groups) == (3 if tail else 2) and all(type(e) is ConvGroup for e in grouped[-len(groups):])
    assert [len(g.convs) for g in groups] == [3, 6, 6][:len(groups)]
    assert all(type(c) is Conv for g in groups for c in g.convs)
    # exactly the default list's entries, the head's regrouped
    assert collections.Counter(flat(grouped)) == collections.Counter(default) and len(flat(grouped)) == len(default)
    # everything outside the head where it was
    assert grouped[:-len(groups)] == default[:-n_head]
    assert len(default) - len(grouped) == (12 if tail else 7)
    assert [c.key for c in groups[0].convs] == [f"det{s}.0" for s in range(3)]
    assert [c.key for c in groups[1].convs] == [f"model.22.cv{b}.{s}.1.conv" for s in range(3) for b in (2, 3)]
    if tail:
        assert [c.key for c in groups[2].convs] == [f"model.22.cv{b}.{s}.2" + (".pad" if b == 3 else "") for s in range(3) for b in (2, 3)]
    assert groups[0].convs[2].srcs[0][0] == "out21" and any(type(e) is not ConvGroup and writes(e)[0][0] == "out21" for e in grouped)


@pytest.mark.parametrize("scale,nc,tail", LISTS)
def test_groups_follow_their_producers_and_members_are_independent(scale, nc, tail):
    grouped = detect_launches(scale, nc, True, tail, True)
    for at, e in enumerate(grouped):
        if type(e) is not ConvGroup:
            continue
        before = [w for p in grouped[:at] for q in (p.convs if type(p) is ConvGroup else (p,)) for w in writes(q)]
        after = [w for p in grouped[at + 1:] for q in (p.convs if type(p) is ConvGroup else (p,)) for w in writes(q)]
        for c in e.convs:
            for r in reads(c):
                assert any(overlap(r, w) for w in before), (c.key, r, "has no producer in front of its group")
                assert not any(overlap(r, w) for w in after), (c.key, r, "is written behind its group")
        for a in e.convs:
            for b in e.convs:
                if a is b:
                    continue
                assert not any(overlap(r, w) for r in reads(a) for w in writes(b)), (a.key, "reads what", b.key, "writes")
                assert not any(overlap(x, w) for x in writes(a) for w in writes(b)), (a.key, "and", b.key, "write the same channels")


@pytest.mark.parametrize("scale,nc,tail", LISTS)
def test_default_list_is_the_parents(scale, nc, tail):
    """The default call, compared with the per-level order REBUILT from the grouped list's Conv fields (not with itself): per level
    det{s}.0, the two .1, (tail) the two .2 - the order the parent walks - behind the unchanged backbone and neck."""
    default = detect_launches(scale, nc, True, tail)
    assert default == detect_launches(scale, nc, fused_c2f=True, tail=tail, grouped_head=False) == detect_launches(scale, nc, True, tail, False)
    grouped = detect_launches(scale, nc, True, tail, True)
    groups = [e.convs for e in grouped if type(e) is ConvGroup]
    rebuilt = [e for e in grouped if type(e) is not ConvGroup]
    for s in range(3):
        rebuilt.append(groups[0][s])
        for g in groups[1:]:
            rebuilt += [Conv(*g[2 * s]), Conv(*g[2 * s + 1])]
    assert tuple(rebuilt) == default
    per = 5 if tail else 3
    keys = [e.key for e in default[-3 * per:]]
    want = []
    for s in range(3):
        want += [f"det{s}.0", f"model.22.cv2.{s}.1.conv", f"model.22.cv3.{s}.1.conv"]
        want += [f"model.22.cv2.{s}.2", f"model.22.cv3.{s}.2.pad"] if tail else []
    assert keys == want
    assert {type(e) for e in default} <= {Stem, Conv, C2fFused, Pool}


# ------------------------------------------------------------------------------------------------------------------ the plan
def Options(**kw):
    """test_gpu_conv_routes.Options (shipped options, restored on exit) with the small-map step's options at their defaults too."""
    return RouteOptions(yvhip, **dict(dict(conv_small=0, conv_small_fill=5, conv_small_rows=0), **kw))


def head_shapes(scale, nc, B, size=640, tail=False):
    """Per ConvGroup of the head: [(key, shape)] with the shape conv2d_group_plan takes."""
    ch, c2, c3, ncp = engines.detect_widths(scale, nc)
    ld = {"hb": c2 + c3, "hc": c2 + c3, "box": 64, "cls": ncp}
    out = []
    for e in detect_launches(scale, nc, True, tail, True):
        if type(e) is ConvGroup:
            out.append([(c.key, (B, size // c.down, size // c.down, c.k, c.stride, c.srcs[0][2], 0, c.cout, ld[c.out.split(".")[1]], 0, c.flags))
                        for c in e.convs])
    return out


def alone(shape):
    return yvhip.conv2d_instance(*shape[:9], res_ld=shape[9], flags=shape[10], ws_bytes=0)


def check_plan(shapes, plan, n_launches):
    """What holds for every plan: each member's instance is its own route; members share a launch only on one groupable instance,
    at most CONV_GROUP_MAX of them; inside a launch they lie in descending work, each first workgroup a multiple of 8 at or behind
    the previous member's end; the launches are numbered without gaps."""
    rows = {yvhip.CONV_DMA_64_3: 128, yvhip.CONV_SMALL_64: 64, yvhip.CONV_SMALL_32: 32}
    by_launch = collections.defaultdict(list)
    for s, p in zip(shapes, plan):
        assert p["instance"] == alone(s), (s, p)
        by_launch[p["launch"]].append((p["position"], s, p))
    assert sorted(by_launch) == list(range(n_launches))
    for members in by_launch.values():
        members.sort(key=lambda m: m[0])
        assert [m[0] for m in members] == list(range(len(members))) and len(members) <= yvhip.CONV_GROUP_MAX
        if len(members) > 1:
            assert len({m[2]["instance"] for m in members}) == 1 and members[0][2]["instance"] & 15 in yvhip.CONV_GROUP_INSTANCES
        end, work = 0, None
        for _, s, p in members:
            if p["instance"] & 15 not in yvhip.CONV_GROUP_INSTANCES:
                assert len(members) == 1 and p["first_wg"] == 0
                continue
            r = rows[p["instance"] & 15]
            M, K = s[0] * s[1] * s[2], s[3] * s[3] * (s[5] + s[6])
            nwg = -(-M // r) * -(-s[7] // 64)
            assert p["work"] == nwg * (K // 64)
            assert p["first_wg"] % 8 == 0 and p["first_wg"] >= end, (p, end)
            assert p["first_wg"] < end + 8                               # (no more padding than the rounding asks for)
            assert work is None or p["work"] <= work, "descending work"
            end, work = p["first_wg"] + nwg, p["work"]


@pytest.mark.parametrize("small", [0, 12800])
@pytest.mark.parametrize("B", [1, 32])
def test_plan_of_the_yolov8n_head(B, small):
    with Options(conv_small=small):
        for step, members in enumerate(head_shapes("n", 5, B, tail=True)):
            keys, shapes = [k for k, _ in members], [s for _, s in members]
            n, plan = yvhip.conv2d_group_plan(shapes)
            check_plan(shapes, plan, n)
            inst = [p["instance"] for p in plan]
            for i in range(len(plan)):                                  # equal groupable instances share a launch (at most 6 members here)
                for j in range(i):
                    if inst[i] == inst[j] and inst[i] & 15 in yvhip.CONV_GROUP_INSTANCES:
                        assert plan[i]["launch"] == plan[j]["launch"], (keys[i], keys[j])
                    else:
                        assert plan[i]["launch"] != plan[j]["launch"], (keys[i], keys[j])
            if step == 0:
                det0 = plan[0]
                if B == 32:                                             # 128-wide, 131,072 pixels: the two-stage 128-wide tiles, alone
                    assert det0["instance"] == yvhip.CONV_DMA_128_2 | yvhip.CONV_STAGED
                    assert [p["launch"] for p in plan].count(det0["launch"]) == 1 and n == 2
                elif small == 0:
                    assert n == 1 and set(inst) == {yvhip.CONV_DMA_64_3 | yvhip.CONV_STAGED}
                else:
                    assert set(inst) <= {yvhip.CONV_SMALL_64, yvhip.CONV_SMALL_32}
            if step == 1 and small == 0:
                assert n == 1 and set(inst) == {yvhip.CONV_DMA_64_3 | yvhip.CONV_STAGED}
            if step == 2:                                               # the 8-wide class logits: igemm_kernel, alone
                assert [p["instance"] & 15 for p in plan[1::2]] == [yvhip.CONV_IGEMM_16] * 3 and n == 1 + 3 + (small > 0 and B == 32)


def test_plan_leaves_igemm_members_single_and_splits_nine_members():
    dma = (1, 9, 9, 3, 1, 64, 0, 64, 64, 0, 0)
    with Options():
        shapes = [dma, (1, 9, 9, 3, 1, 24, 0, 64, 64, 0, 0), dma, (1, 9, 9, 3, 1, 64, 0, 16, 16, 0, 0), dma]
        n, plan = yvhip.conv2d_group_plan(shapes)
        check_plan(shapes, plan, n)
        assert n == 3 and [p["launch"] for p in plan] == [0, 1, 0, 2, 0]
        assert [p["instance"] & 15 for p in plan] == [yvhip.CONV_DMA_64_3, yvhip.CONV_IGEMM_64, yvhip.CONV_DMA_64_3, yvhip.CONV_IGEMM_16,
                                                      yvhip.CONV_DMA_64_3]
        nine = [(1, 10 * (i + 1), 13, 3, 1, 64, 0, 64, 64, 0, 0) for i in range(9)]                 # 2, 3, .. 10 tiles of 128 pixels
        n, plan = yvhip.conv2d_group_plan(nine)
        check_plan(nine, plan, n)
        assert n == 2 and sorted(p["launch"] for p in plan) == [0] * 8 + [1]
        assert plan[0]["launch"] == 1 and plan[0]["first_wg"] == 0       # the lightest member is the one left over
        n, plan = yvhip.conv2d_group_plan([dma])
        assert n == 1 and plan == [dict(launch=0, instance=yvhip.CONV_DMA_64_3 | yvhip.CONV_STAGED, first_wg=0, position=0, work=9)]
    for rows, code in ((64, yvhip.CONV_SMALL_64), (32, yvhip.CONV_SMALL_32)):
        with Options(conv_small=1 << 20, conv_small_fill=1 << 20, conv_small_rows=rows):
            big = (1, 17, 17, 1, 1, 64, 0, 128, 128, 0, 0)
            shapes = [dma, big, (1, 9, 9, 3, 1, 128, 0, 128, 128, 0, 0)]
            n, plan = yvhip.conv2d_group_plan(shapes)
            check_plan(shapes, plan, n)
            assert n == 1 and {p["instance"] for p in plan} == {code}
            assert plan[1]["first_wg"] > 0 and (289 + rows - 1) // rows * 2 % 8 != 0


def test_plan_rejects_what_the_launch_rejects():
    with pytest.raises(yvhip.YvError):
        yvhip.conv2d_group_plan([])
    with pytest.raises(yvhip.YvError):
        yvhip.conv2d_group_plan([(1, 9, 9, 3, 1, 64, 0, 64, 64, 0, 0), (1, 9, 9, 5, 1, 64, 0, 64, 64, 0, 0)])       # ksize 5
    with pytest.raises(yvhip.YvError):
        yvhip.conv2d_group_plan([(1, 9, 9, 3, 1, 60, 0, 64, 64, 0, 0)])                                            # Cin % 8
