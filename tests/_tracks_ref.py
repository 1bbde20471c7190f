"""numpy statement of the rip tracks (rcflow_tracks_*), written from the contract in include/rcflow.h, steps 0 to 7, not from
the kernels: plain loops over labels and slots, int64 and Python integers throughout.  It takes the label image and the records of a
regions push (for instance from _regions_ref.regions) and keeps the state from push to push."""
import numpy as np

TRACK = np.dtype([("id", "<i8"), ("parent", "<i8"), ("first_push", "<i8"), ("area_sum", "<i8"), ("fx_sum", "<i8"), ("fy_sum", "<i8"),
                  ("m_sum", "<i8"), ("slot", "<i4"), ("label", "<i4"), ("flags", "<i4"), ("age", "<i4"), ("hits", "<i4"),
                  ("misses", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("px", "<i4"),
                  ("py", "<i4"), ("px0", "<i4"), ("py0", "<i4"), ("overlap", "<i4"), ("mean_fx", "<f4"), ("mean_fy", "<f4")])
PRIM = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"),
                 ("color", "<u4"), ("flags", "<u4")])
DISC, LINE = 1, 2
SEEN, BORN, COASTING, ENDED, SPLIT, MERGED, CONFIRMED = 1, 2, 4, 8, 16, 32, 64


def _mean(total, m):
    """(float)((double)total / 65536 / m), each operation rounded on its own; 0 when m is 0"""
    return np.float32(np.float64(total) / np.float64(65536.0) / np.float64(m)) if m else np.float32(0)


class Tracks:
    def __init__(self, w, h, max_regions=1024, max_tracks=64, min_overlap=1, max_misses=2, min_hits=3):
        self.w, self.h = w, h
        self.max_regions, self.max_tracks, self.min_overlap, self.max_misses, self.min_hits = max_regions, max_tracks, min_overlap, max_misses, min_hits
        self.reset()

    def reset(self):
        self.P = np.zeros((self.h, self.w), np.int32)
        self.tab = np.zeros(self.max_tracks, TRACK)
        self.next_id, self.n = 1, 0
        self.summary = np.zeros(8, np.int64)

    def _seen_as(self, q, r):
        """the geometry and the sums a track takes from the record of the region it is seen as"""
        n = int(r["area"])
        for k in ("area", "x0", "y0", "x1", "y1"):
            q[k] = r[k]
        q["px"], q["py"] = ((2 * int(r["sx"]) + n) // (2 * n), (2 * int(r["sy"]) + n) // (2 * n)) if n > 0 else (0, 0)   # n >= 1 in a written record
        q["area_sum"] += n
        q["fx_sum"] += int(r["fx"])
        q["fy_sum"] += int(r["fy"])
        q["m_sum"] += n - int(r["bad"])

    def push(self, labels, records, written):
        """labels: h x w integers; records: the rc_region records (record c is records[c - 1]); written: summary[2] of the regions
        push.  -> dict(tracks, track_of_label, mask_out, summary, footprint), all copies"""
        labels = np.asarray(labels).astype(np.int64)
        assert labels.shape == (self.h, self.w)
        T, NR = self.max_tracks, self.max_regions
        R = min(max(int(written), 0), NR)
        self.n += 1
        tab, P = self.tab, self.P
        # 0. free
        for t in range(T):
            if tab[t]["flags"] & ENDED:
                tab[t] = np.zeros((), TRACK)
        alive = [t for t in range(T) if tab[t]["id"] != 0]
        # 1. overlap
        inside = (labels >= 1) & (labels <= R)
        sel = inside & (P > 0)
        ov = np.bincount(labels[sel] * T + (P[sel].astype(np.int64) - 1), minlength=(NR + 1) * T).reshape(NR + 1, T)
        # 2. claim
        best = {}
        al = np.array(alive, np.int64)
        ids = tab["id"][al]
        for c in range(1, R + 1):
            o = ov[c, al]
            ok = o >= self.min_overlap
            if ok.any():
                best[c] = int(al[ok][np.lexsort((ids[ok], -o[ok]))[0]])   # the largest overlap, the smaller id among equals
        # 3. winner
        claimed = {}
        for c in sorted(best):
            claimed.setdefault(best[c], []).append(c)
        winner, claims = {}, {}
        for t in alive:
            cs = claimed.get(t, [])
            claims[t] = len(cs)
            if cs:
                winner[t] = min(cs, key=lambda c: (-int(ov[c, t]), c))
        # 4. update
        slot_of = {}
        for t in alive:
            q = tab[t]
            q["age"] += 1
            if t in winner:
                c = winner[t]
                q["flags"] = SEEN | (SPLIT if claims[t] > 1 else 0)
                q["hits"] += 1
                q["misses"], q["label"], q["overlap"] = 0, c, ov[c, t]
                self._seen_as(q, records[c - 1])
                slot_of[c] = t
            else:
                q["flags"] = COASTING | (MERGED if (ov[1:R + 1, t] >= self.min_overlap).any() else 0)
                q["misses"] += 1
                q["label"], q["overlap"] = 0, 0
                if q["misses"] > self.max_misses:
                    q["flags"] |= ENDED
            if q["hits"] >= self.min_hits:
                q["flags"] |= CONFIRMED
            q["mean_fx"], q["mean_fy"] = _mean(int(q["fx_sum"]), int(q["m_sum"])), _mean(int(q["fy_sum"]), int(q["m_sum"]))
        n_ended = sum(1 for t in alive if tab[t]["flags"] & ENDED)
        n_coast = sum(1 for t in alive if tab[t]["flags"] & COASTING)
        # 5. births
        free = [t for t in range(T) if tab[t]["id"] == 0]
        orphans = [c for c in range(1, R + 1) if c not in slot_of]
        born = min(len(free), len(orphans))
        for k in range(born):
            c, t = orphans[k], free[k]
            q = np.zeros((), TRACK)
            q["id"] = self.next_id + k
            q["parent"] = tab[best[c]]["id"] if c in best else 0
            q["first_push"], q["slot"], q["label"] = self.n, t, c
            q["flags"] = BORN | SEEN | (CONFIRMED if self.min_hits <= 1 else 0)
            q["age"] = q["hits"] = 1
            self._seen_as(q, records[c - 1])
            q["px0"], q["py0"] = q["px"], q["py"]
            q["mean_fx"], q["mean_fy"] = _mean(int(q["fx_sum"]), int(q["m_sum"])), _mean(int(q["fy_sum"]), int(q["m_sum"]))
            tab[t] = q
            slot_of[c] = t
        self.next_id += born
        # 6. paint
        tol = np.zeros(NR + 1, np.int32)
        for c, t in slot_of.items():
            tol[c] = t + 1
        goes_on = np.zeros(T + 1, bool)
        for t in alive:
            goes_on[t + 1] = not (tab[t]["flags"] & ENDED)
        self.P = np.where(inside, tol[np.where(inside, labels, 0)], np.where(goes_on[P], P, 0)).astype(np.int32)
        # 7. outputs
        conf = np.zeros(NR + 1, bool)
        for c, t in slot_of.items():
            conf[c] = bool(tab[t]["flags"] & CONFIRMED)
        mask = np.where(inside & conf[np.where(inside, labels, 0)], 255, 0).astype(np.uint8)
        live = [t for t in range(T) if tab[t]["id"] != 0 and not (tab[t]["flags"] & ENDED)]
        self.summary = np.array([len(live), sum(1 for t in live if tab[t]["flags"] & CONFIRMED), born, n_ended,
                                 sum(1 for t in live if tab[t]["flags"] & SEEN), n_coast, len(orphans) - born, self.n], np.int64)
        return dict(tracks=tab.copy(), track_of_label=tol, mask_out=mask, summary=self.summary.copy(), footprint=self.P.copy())


def prims(tracks, color=0x00ffff, thickness=1, disc_radius=3):
    """the 5 primitives per slot of rcflow_tracks_prims_dev"""
    q = np.asarray(tracks)
    out = np.zeros((len(q), 5), PRIM)
    x0, y0, x1, y1 = (q[k].astype(np.int64) for k in ("x0", "y0", "x1", "y1"))
    for j, (a, b, c, d) in enumerate(((x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0))):
        out["kind"][:, j], out["size"][:, j], out["color"][:, j] = LINE, thickness, color
        out["x0"][:, j], out["y0"][:, j], out["x1"][:, j], out["y1"][:, j] = a, b, c, d
    out["kind"][:, 4], out["size"][:, 4], out["color"][:, 4] = DISC, disc_radius, color
    out["x0"][:, 4] = out["x1"][:, 4] = q["px"]
    out["y0"][:, 4] = out["y1"][:, 4] = q["py"]
    shown = ((q["flags"] & CONFIRMED) != 0) & ((q["flags"] & ENDED) == 0)
    out[~shown] = np.zeros((), PRIM)
    return out.reshape(-1)
