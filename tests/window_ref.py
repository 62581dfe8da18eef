"""CPU references for rudp_accept_window / rudp_gather_ordered.

``window_ref``: the reordering receiver's rule (include/rudp.h) as a plain loop
over the frames, the pending set a dict.
``ordered_ref``: payloads out in rank order, in numpy.
``chunk_model``: the device's form in plain Python -- chunks of 1024 new frames
plus the frames pending before them, every reset segment's chain found from
the sorted candidates, the delivery times a prefix maximum -- with the index
where it hands over to the sequential walk (``info[4]``).
``window_stream``: what a windowed cumulative sender leaves at a receiver
under loss, duplication and adjacent swaps; ``adversarial_window_stream``:
random frames in a band a few windows wide.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

SYN, ACK, FIN = 0x80, 0x40, 0x20
NO_ISN = 0xFFFFFFFF
NONE = 0xFFFFFFFF
CHUNK = 1024          # new frames per launch of the device form
ST_OFFSETS, ST_PAYLOAD_CAP, ST_RANK = 8, 16, 64


class WindowResult(NamedTuple):
    accept: np.ndarray       # u8 [n]: 1 delivered, 2 pending at the end
    rank: np.ndarray         # u32 [n]
    carry_rank: np.ndarray   # u32 [n]
    reply: np.ndarray        # u8 [n]
    reply_ack: np.ndarray    # u16 [n]
    state: tuple             # (expect, isn, live)
    info: list               # end, K, msg_start, characters, first_anomaly, pending, delivered, 0


def _finish(n, accept, order, pending, reply, ack, expect, isn, live, end, ms, first_anomaly):
    rank = np.full(n, NONE, np.uint32)
    carry = np.full(n, NONE, np.uint32)
    for k, j in enumerate(order):
        rank[j] = k
    for k, j in enumerate(sorted(pending)):
        carry[j] = k
    info = [end, len(order), ms, expect - isn if live else 0, first_anomaly, len(pending),
            int((accept == 1).sum()), 0]
    return WindowResult(accept, rank, carry, reply, ack, (expect, isn, live), info)


def window_ref(seq, flags, chars, usable=None, state=(0, 0, 0), last_isn: Optional[int] = None, *,
               window_chars: int, n_carried: int = 0) -> WindowResult:
    n = len(seq)
    Wc = int(window_chars)
    expect, isn, live = int(state[0]), int(state[1]), 1 if state[2] else 0
    last = NO_ISN if last_isn is None else int(last_isn)
    accept = np.zeros(n, np.uint8)
    reply = np.zeros(n, np.uint8)
    ack = np.zeros(n, np.uint16)
    P = {}       # start -> frame index
    order = []   # delivered frames since the last reset
    end, ms = n, n
    for i in range(n):
        if usable is not None and not usable[i]:
            continue
        s, f, c = int(seq[i]), int(flags[i]), int(chars[i])
        fin = False
        if f & SYN:
            if s != last:
                isn, expect, live, ms = s, s + c, 1, i
                for j in P.values():
                    accept[j] = 0
                P.clear()
                order = [i]
                accept[i] = 1
                fin = bool(f & FIN)
        elif live and s == expect:
            accept[i] = 1
            order.append(i)
            expect += c
            fin = bool(f & FIN)
            while not fin and expect in P:
                j = P.pop(expect)
                accept[j] = 1
                order.append(j)
                expect += int(chars[j])
                fin = bool(int(flags[j]) & FIN)
            for st in [st for st in P if st < expect]:
                accept[P.pop(st)] = 0
        elif live and expect < s < expect + Wc and c > 0 and s not in P:
            P[s] = i
            accept[i] = 2
        if live and i >= n_carried:
            reply[i] = 1
            ack[i] = expect & 0xFFFF
        if fin:
            end = i
            for j in P.values():
                accept[j] = 0
            P.clear()
            break
    return _finish(n, accept, order, list(P.values()), reply, ack, expect, isn, live, end, ms, n)


def ordered_ref(frames, frame_off, rank, count, skip, out_cap=None):
    """(out bytes, out_off int64 [K + 1], src int64 [K], status): frame i with
    rank r < K puts max(len_i - skip, 0) bytes at out_off[r]."""
    frames = np.asarray(frames, np.uint8)
    K = min(int(count), len(frame_off) - 1)  # (a count above n counts as n)
    src = np.full(K, -1, np.int64)
    status = 0
    for i, r in enumerate(np.asarray(rank, np.uint32).tolist()):
        if r == NONE:
            continue
        if r >= K:
            status |= ST_RANK
            continue
        src[r] = i
    parts = []
    for k in range(K):
        i = int(src[k])
        piece = b""
        if i >= 0:
            a, b = int(frame_off[i]), int(frame_off[i + 1])
            if not (0 <= a <= b <= len(frames)):
                status |= ST_OFFSETS
            elif b - a > skip:
                piece = frames[a + skip:b].tobytes()
        parts.append(piece)
    off = np.zeros(K + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    if out_cap is not None and off[K] > out_cap:
        status |= ST_PAYLOAD_CAP
    return np.frombuffer(b"".join(parts), np.uint8), off, src, status


# -------------------------------------------------------------- device model
def _lower_bound(keys, lo, hi, v):
    while lo < hi:
        m = (lo + hi) >> 1
        if keys[m] < v:
            lo = m + 1
        else:
            hi = m
    return lo


def chunk_model(seq, flags, chars, usable=None, state=(0, 0, 0), last_isn: Optional[int] = None, *,
                window_chars: int, n_carried: int = 0) -> WindowResult:
    """csrc/window.hip step by step.  Equal to ``window_ref`` in every output
    but ``info[4]``, the first frame a chunk gave to the sequential walk."""
    n, Wc = len(seq), int(window_chars)
    last = NO_ISN if last_isn is None else int(last_isn)
    seq = [int(v) for v in seq]
    flags = [int(v) for v in flags]
    chars = [int(v) for v in chars]
    us = [1] * n if usable is None else [1 if v else 0 for v in usable]
    accept = np.zeros(n, np.uint8)
    rank = np.full(n, NONE, np.uint32)
    reply = np.zeros(n, np.uint8)
    ack = np.zeros(n, np.uint16)
    E, isn, live = int(state[0]), int(state[1]), 1 if state[2] else 0
    rb, dc, ms, end, first = 0, 0, n, n, n
    car = list(range(n_carried))
    new0 = n_carried
    chunk = 0
    while True:
        new1 = min(n, new0 + CHUNK)
        it = car + list(range(new0, new1))
        ncar, M = len(car), len(car) + new1 - new0
        # 1. classes and segments
        cls = []
        for p in it:
            if not us[p]:
                cls.append(0)
            elif flags[p] & SYN:
                cls.append(1 if seq[p] == last else 2)
            else:
                cls.append(3)
        seg, segpos, g = [], [None], 0
        for p in range(M):
            if cls[p] == 2:
                g += 1
                segpos.append(p)
            seg.append(g)

        def E0(g):
            return E if g == 0 else seq[it[segpos[g]]] + chars[it[segpos[g]]]

        def lv(g):
            return 1 if g else live
        # 2. candidates sorted by (segment, seq, arrival)
        keys = sorted((seg[p] << 27) | (seq[it[p]] << 11) | p for p in range(M)
                      if cls[p] == 3 and chars[it[p]] > 0 and lv(seg[p]) and seq[it[p]] >= E0(seg[p]))
        Nc = len(keys)
        pos2q = [None] * M
        for q, k in enumerate(keys):
            pos2q[k & 2047] = q
        # 3. first arrival per start, successors, the chains by pointer doubling
        node = [q == 0 or keys[q - 1] >> 11 != keys[q] >> 11 for q in range(Nc)]

        def find(g, t):
            if t > 65535:
                return None
            lb = _lower_bound(keys, 0, Nc, (g << 27) | (t << 11))
            return lb if lb < Nc and keys[lb] >> 11 == (g << 16) | t else None
        succ = [None] * Nc
        for q in range(Nc):
            p = it[keys[q] & 2047]
            if node[q] and not flags[p] & FIN:
                succ[q] = find(keys[q] >> 27, seq[p] + chars[p])
        mark = [False] * Nc
        for g in range(len(segpos)):
            if lv(g):
                r = find(g, E0(g))
                if r is not None:
                    mark[r] = True
        for _ in range(11):
            for q in [q for q in range(Nc) if mark[q] and succ[q] is not None]:
                mark[succ[q]] = True
            succ = [succ[s] if s is not None else None for s in succ]
        # 4. the chain elements in order, their delivery times
        cq = [q for q in range(Nc) if mark[q]]
        cD, run = [], 0
        for q in cq:
            run = max(run, (keys[q] >> 27) << 11 | (keys[q] & 2047))
            cD.append(run)
        q2j = {q: j for j, q in enumerate(cq)}

        def nextE(j):
            p = it[keys[cq[j]] & 2047]
            return seq[p] + chars[p]

        def guess(p, after):
            g = seg[p]
            cnt = _lower_bound(cD, 0, len(cD), ((g << 11) | p) + (1 if after else 0))
            if cnt and cD[cnt - 1] >> 11 == g:
                return nextE(cnt - 1), cnt
            return E0(g), cnt

        def jlo(g):
            return _lower_bound(cD, 0, len(cD), g << 11)
        # 5. every item under the guess
        st, rk, rep, ak, pend = [0] * M, [NONE] * M, [0] * M, [0] * M, [False] * M
        pe, pa = M, M
        for p in range(M):
            i, g = it[p], seg[p]
            Gb, _ = guess(p, False)
            Ga, _ = guess(p, True)
            if cls[p] == 2:
                st[p], rk[p] = 1, 0
                if flags[i] & FIN:
                    pe = min(pe, p)
            elif cls[p] == 3 and lv(g):
                s, c = seq[i], chars[i]
                if (s == Gb and c == 0) or (c > 0 and s >= Gb + Wc):
                    pa = min(pa, p)
                q = pos2q[p]
                if q is not None and node[q] and Gb < s < Gb + Wc:
                    pend[p] = True
                if q is not None and mark[q]:
                    j = q2j[q]
                    st[p], rk[p] = 1, (1 if g else rb) + j - jlo(g)
                    if flags[i] & FIN:
                        pe = min(pe, cD[j] & 2047)
                elif pend[p]:
                    st[p] = 2
            if cls[p] and lv(g) and p >= ncar:
                rep[p], ak[p] = 1, Ga & 0xFFFF
        if pa < pe:
            # 7. the walk from the exact state before pa
            first = min(first, it[pa])
            g = seg[pa]
            Eb, cnt = guess(pa, False)
            ring = [None] * Wc
            for p in range(pa):
                q = pos2q[p]
                if cls[p] == 2:
                    continue
                if q is not None and mark[q] and (cD[q2j[q]] & 2047) < pa:
                    continue
                st[p], rk[p] = 0, NONE
                if pend[p] and seg[p] == g and seq[it[p]] > Eb:
                    st[p] = 2
                    ring[seq[it[p]] % Wc] = p
            r = (1 if g else rb) + cnt - jlo(g)
            dc += g + cnt
            if g:
                isn, ms = seq[it[segpos[g]]], it[segpos[g]]
            E, live, pe = Eb, 1, M

            def clear():
                for w in range(Wc):
                    if ring[w] is not None:
                        st[ring[w]] = 0
                        ring[w] = None

            def advance(old, new):
                for s in range(old + 1, min(new, old + Wc)):
                    w = s % Wc
                    if ring[w] is not None:
                        st[ring[w]] = 0
                        ring[w] = None
            for p in range(pa, M):
                i = it[p]
                st[p], rk[p], rep[p], ak[p] = 0, NONE, 0, 0
                if not cls[p]:
                    continue
                s, f, c = seq[i], flags[i], chars[i]
                fin = False
                if cls[p] == 2:
                    isn, E, live, ms = s, s + c, 1, i
                    clear()
                    st[p], rk[p], r = 1, 0, 1
                    dc += 1
                    fin = bool(f & FIN)
                elif cls[p] == 3 and live and s == E:
                    st[p], rk[p] = 1, r
                    r += 1
                    dc += 1
                    fin = bool(f & FIN)
                    if c:
                        advance(E, E + c)
                        E += c
                        while not fin and ring[E % Wc] is not None:
                            j = ring[E % Wc]
                            ring[E % Wc] = None
                            st[j], rk[j] = 1, r
                            r += 1
                            dc += 1
                            fin = bool(flags[it[j]] & FIN)
                            advance(E, E + chars[it[j]])
                            E += chars[it[j]]
                elif cls[p] == 3 and live and E < s < E + Wc and c > 0 and ring[s % Wc] is None:
                    ring[s % Wc] = p
                    st[p] = 2
                if live and p >= ncar:
                    rep[p], ak[p] = 1, E & 0xFFFF
                if fin:
                    pe = p
                    clear()
                    break
            rb = r
        else:
            # 6. the guess was exact up to the end
            if M:
                pl = min(pe, M - 1)
                g = seg[pl]
                E_new, cnt = guess(pl, True)
                if lv(g):
                    E = E_new
                rb = (1 if g else rb) + cnt - jlo(g)
                dc += g + cnt
                if g:
                    isn, ms, live = seq[it[segpos[g]]], it[segpos[g]], 1
                for p in range(M):
                    if st[p] == 2 and not (pe == M and seg[p] == g and seq[it[p]] > E):
                        st[p] = 0
        # 8. outputs
        car = []
        for p in range(M):
            i = it[p]
            if p > pe:
                accept[i], rank[i], reply[i], ack[i] = 0, NONE, 0, 0
                continue
            accept[i], rank[i] = st[p], rk[p] if st[p] == 1 else NONE
            if p >= ncar or chunk == 0:
                reply[i], ack[i] = rep[p], ak[p]
            if st[p] == 2:
                car.append(i)
        if pe < M:
            end = it[pe]
            break
        new0 = new1
        chunk += 1
        if new0 >= n:
            break
    for i in range(n):
        if i > end:
            accept[i], rank[i], reply[i], ack[i] = 0, NONE, 0, 0
        elif i < ms < n:
            rank[i] = NONE
    order = sorted((int(r), i) for i, r in enumerate(rank.tolist()) if r != NONE)
    assert [r for r, _ in order] == list(range(len(order))), "ranks are not a permutation"
    res = _finish(n, accept, [i for _, i in order], car, reply, ack, E, isn, live, end, ms, first)
    assert res.info[1] == rb and res.info[6] == dc, (res.info, rb, dc)
    return res


# ------------------------------------------------------------------- streams
def window_stream(rng, n, W, C, p_loss=0.05, p_dup=0.02, p_swap=0.05, *, total=None, isn=None, syn=True,
                  p_unusable=0.0):
    """n frames a sender with W frames of C characters in flight and cumulative
    acknowledgements leaves at a receiver with a window of W * C characters:
    rounds of the unsent frames of [base, base + W), each lost, doubled or
    swapped with its neighbour in flight, base moved to the receiver's
    cumulative ack after every round, and the whole window sent again after a
    round without progress (go-back-N).  No frame is ever at or beyond the
    receiver's expect + W * C.  The SYN is frame 0 (never doubled: a second
    copy restarts the transfer); ``syn=False`` starts at frame 1 of a transfer
    whose SYN an earlier batch took.  ``total``: frames of the message, the
    last one with FIN (None: longer than the stream).
    Returns seq (u16), flags (u8), chars (u32), usable (u8), state."""
    isn = rng.randint(1, 3000) if isn is None else isn
    seq = np.zeros(n, np.uint16)
    flags = np.zeros(n, np.uint8)
    chars = np.full(n, C, np.uint32)
    usable = np.ones(n, np.uint8)
    first = 0 if syn else 1
    base = exp = first          # sender's base, receiver's next frame
    have = set()
    live = not syn
    sent_to = base              # frames below it went out in this window
    k = 0
    while k < n:
        hi = base + W if total is None else min(base + W, total)
        if sent_to >= hi:       # nothing new to send and no progress: the window again
            sent_to = base
        flight = []
        for fr in range(sent_to, hi):
            if rng.random() < p_loss:
                continue
            flight.append(fr)
            if fr and rng.random() < p_dup:
                flight.append(fr)
        sent_to = hi
        for a in range(len(flight) - 1):
            if rng.random() < p_swap:
                flight[a], flight[a + 1] = flight[a + 1], flight[a]
        for fr in flight:
            if k >= n:
                break
            seq[k] = (isn + fr * C) & 0xFFFF
            flags[k] = (SYN if fr == 0 else 0) | (FIN if total is not None and fr == total - 1 else 0)
            if rng.random() < p_unusable:
                usable[k] = 0
            k += 1
            if not usable[k - 1]:
                continue
            if fr == 0:
                live, exp, have = True, 1, set()
            elif live and exp <= fr < exp + W:
                have.add(fr)
            while exp in have:
                have.discard(exp)
                exp += 1
        if live and exp > base:
            base = sent_to = exp
            if total is not None and base >= total:
                base = sent_to = first      # the transfer again (frames behind `end` are not judged)
    state = (0, 0, 0) if syn else (isn + C, isn, 1)
    return seq, flags, chars, usable, state


def adversarial_window_stream(rng, n, Wc, *, span=None, p_syn=0.03, p_fin=0.005, max_chars=3):
    """accept_ref.adversarial_stream in a band a few windows wide: frames from
    the past, ahead inside and beyond the window, repeated starts with other
    lengths, characters 0..max_chars, competing SYNs, seq_num near 65535."""
    span = 3 * Wc + 9 if span is None else span
    base = rng.choice((0, 100, 65530 - span // 2))
    seq = np.array([(base + rng.randint(0, span)) & 0xFFFF for _ in range(n)], np.uint16)
    flags = np.array([(SYN if rng.random() < p_syn else 0) | (FIN if rng.random() < p_fin else 0)
                      | (ACK if rng.random() < 0.1 else 0) for _ in range(n)], np.uint8)
    chars = np.array([rng.randint(0, max_chars) for _ in range(n)], np.uint32)
    usable = np.array([rng.random() > 0.1 for _ in range(n)], np.uint8)
    return seq, flags, chars, usable
