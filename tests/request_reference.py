"""Numpy statement of the packed result record of yv_pack_results (include/yv_hip.h), of the crop list it joins, and of the loop
of inferdet.main it replaces.  Shared by tests/test_request_cpu.py (which checks it against main's own loop) and
tests/test_gpu_request.py (which checks the kernel and the sessions against it)."""
import numpy as np

FIELDS = 9                                   # image, slot, box x 4, det_label, cls_label, score bits; nc logits follow


def compact_ref(det_count, crop_rect, crop_ok, cap):
    """yv_compact_crops: rows {image, x0, y0, x1, y1, slot} of the detections with a valid crop, image ascending, then slot;
    -> (crop_list (max(cap, 1), 6) i32 zero padded, total)."""
    rows = [[b, *np.asarray(crop_rect)[b, k].tolist(), k] for b in range(len(det_count)) for k in range(int(det_count[b]))
            if int(crop_ok[b][k])]
    rows = rows[:cap]
    out = np.zeros((max(cap, 1), 6), dtype=np.int32)
    if rows:
        out[:len(rows)] = np.asarray(rows, dtype=np.int32)
    return out, len(rows)


def pack_ref(crop_list, crop_total, det_box, det_score, det_label, cls_label, cls_logits, cap):
    """-> (1 + cap, 9 + nc) int32 words: row 0 {total, B, slots, cap, nc, 0, ...}; row 1 + k the record of crop k; zero beyond."""
    crop_list, det_box = np.asarray(crop_list, dtype=np.int32), np.asarray(det_box, dtype=np.int32)
    det_score, cls_logits = np.asarray(det_score, dtype=np.float32), np.asarray(cls_logits, dtype=np.float32)
    det_label, cls_label = np.asarray(det_label, dtype=np.int32), np.asarray(cls_label, dtype=np.int32)
    (B, slots), nc = det_score.shape, cls_logits.shape[1]
    total = min(int(np.asarray(crop_total).reshape(-1)[0]), cap)
    out = np.zeros((1 + cap, FIELDS + nc), dtype=np.int32)
    out[0, :5] = (total, B, slots, cap, nc)
    for k in range(total):
        image, slot = int(crop_list[k, 0]), int(crop_list[k, 5])
        out[1 + k, 0:2] = (image, slot)
        out[1 + k, 2:6] = det_box[image, slot]
        out[1 + k, 6:8] = (det_label[image, slot], cls_label[k])
        out[1 + k, 8] = det_score[image, slot:slot + 1].view(np.int32)[0]
        out[1 + k, 9:] = cls_logits[k].view(np.int32)
    return out


def main_loop(det_count, det_box, det_score, det_label, crop_list, crop_total, cls_label):
    """The loop of inferdet.main over cls_of, as it stood before the records: per image the (slot, class, det_label, score,
    box) of its detections that have a classified crop, in score order."""
    cls_of = {(int(crop_list[k][0]), int(crop_list[k][5])): int(cls_label[k]) for k in range(int(crop_total))}
    per_image = []
    for i in range(len(det_count)):
        objs = []
        for k in range(int(det_count[i])):
            c = cls_of.get((i, k))
            if c is None:
                continue
            objs.append((k, c, int(det_label[i][k]), float(det_score[i][k]), [int(v) for v in det_box[i][k]]))
        per_image.append(objs)
    return per_image


def records_per_image(rec, B):
    """unpack_results' dict in main_loop's form."""
    per_image = [[] for _ in range(B)]
    for k in range(len(rec["image"])):
        per_image[int(rec["image"][k])].append((int(rec["slot"][k]), int(rec["cls_label"][k]), int(rec["det_label"][k]),
                                                float(rec["score"][k]), rec["box"][k].tolist()))
    return per_image


def hand_made(nc=5):
    """B = 3, slots = 4: image 0 has three detections, the middle one with crop_ok = 0; image 1 has none; image 2 has two.  Four
    crops; arrays beyond the counts hold a pattern that must not show."""
    B, slots = 3, 4
    det_count = np.array([3, 0, 2], dtype=np.int32)
    det_box = (np.arange(B * slots * 4, dtype=np.int32).reshape(B, slots, 4) * 3 + 1)
    det_score = (0.95 - 0.07 * np.arange(B * slots, dtype=np.float32)).reshape(B, slots)
    det_label = (np.arange(B * slots, dtype=np.int32).reshape(B, slots) * 7) % nc
    crop_rect = det_box + np.array([-2, -2, 2, 2], dtype=np.int32)
    crop_ok = np.ones((B, slots), dtype=np.int32)
    crop_ok[0, 1] = 0
    return dict(B=B, slots=slots, nc=nc, det_count=det_count, det_box=det_box, det_score=det_score, det_label=det_label,
                crop_rect=crop_rect, crop_ok=crop_ok)


def classifier_outputs(cap, nc, seed=7):
    g = np.random.default_rng(seed)
    logits = g.standard_normal((max(cap, 1), nc)).astype(np.float32)
    return logits.argmax(1).astype(np.int32), logits
