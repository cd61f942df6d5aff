"""A numpy oracle of the Mode S / ADS-B decoder, written from DESIGN.md section 17 and independent of the package: the
plan, the quantiser, the chip sums, the preamble rule, the slicer and the 24-bit check over every sample position, the host
logic (grouping, identification, position with global CPR, velocity, the aircraft table), a frame builder that appends the
parity, and a PPM modulator that integrates the ideal pulse train over each sample period (a box front end) with a
sub-sample start, a carrier offset and complex noise."""
from __future__ import annotations

import math

import numpy as np

RATES = [2.0e6, 2.4e6, 2.5e6, 4.0e6, 10.0e6, 20.0e6]
OFFSETS = [0.0, 0.25, 0.5, 0.75]
CARRIERS = [0.0, 50e3]
SIGMAS = [0.0, 0.05, 0.1]
GENERATOR = 0x1FFF409
CHIPS = 240
CHARSET = "#ABCDEFGHIJKLMNOPQRSTUVWXYZ#####_###############0123456789######"

IDENT = bytes.fromhex("8D4840D6202CC371C32CE0576098")
POS_EVEN = bytes.fromhex("8D40621D58C382D690C8AC2863A7")
POS_ODD = bytes.fromhex("8D40621D58C386435CC412692AD6")
VELOCITY = bytes.fromhex("8D485020994409940838175B284F")
VELOCITY_3 = bytes.fromhex("8DA05F219B06B6AF189400CBC33F")
PUBLISHED = [IDENT, POS_EVEN, POS_ODD, VELOCITY, VELOCITY_3]


# ---- the plan -------------------------------------------------------------------------------------------------------------


def plan(fs: float) -> dict:
    sps = float(fs) / 1e6
    if not 2.0 <= sps <= 20.0:
        raise ValueError("sps outside 2 .. 20")
    h = int(math.floor(sps / 2.0))
    o = np.rint(np.arange(CHIPS, dtype=np.float64) * (sps / 2.0)).astype(np.int64)
    return dict(fs=float(fs), sps=sps, h=h, o=o, span=int(o[-1]) + h, L=int(np.rint(sps)))


# ---- frames ---------------------------------------------------------------------------------------------------------------


def syndrome(data: bytes) -> int:
    """Long division, bit by bit: the remainder of the whole bit string under the 25-bit generator."""
    value = int.from_bytes(data, "big")
    nbits = 8 * len(data)
    for k in range(nbits - 1, 23, -1):
        if (value >> k) & 1:
            value ^= GENERATOR << (k - 24)
    return value


def with_parity(body: bytes) -> bytes:
    return body + syndrome(body + b"\0\0\0").to_bytes(3, "big")


def build_frame(df: int, icao: int, me: int | None = None, ca: int = 5) -> bytes:
    """DF11 (``me`` None; interrogator code 0), DF17 or DF18 with a 56-bit ``me``, the parity appended."""
    head = bytes([(df << 3) | ca]) + icao.to_bytes(3, "big")
    if df == 11:
        assert me is None
        return with_parity(head)
    assert df in (17, 18, 19) and me is not None
    return with_parity(head + me.to_bytes(7, "big"))


DF11 = build_frame(11, 0x4840D6)
FOUR = [IDENT, POS_EVEN, POS_ODD, DF11]  # one identification, an even / odd pair, one DF11


def chips_of(frame: bytes) -> np.ndarray:
    """The 0 / 1 amplitude of the half-microsecond chips: 16 of the preamble, two per bit (1: pulse first)."""
    a = np.zeros(16 + 16 * len(frame), dtype=np.float64)
    a[[0, 2, 7, 9]] = 1.0
    bits = np.unpackbits(np.frombuffer(frame, dtype=np.uint8))
    a[16 + 2 * np.arange(bits.size) + (1 - bits)] = 1.0
    return a


def pulse_samples(frame: bytes, fs: float, frac: float, count: int) -> np.ndarray:
    """``count`` samples of the frame's ideal pulse train, started ``frac`` of a sample behind sample 0, each the mean of
    the train over its sample period."""
    a = chips_of(frame)
    knots = np.arange(a.size + 1, dtype=np.float64) * 0.5e-6
    integral = np.concatenate(([0.0], np.cumsum(a) * 0.5e-6))
    ts = 1.0 / fs
    edges = (np.arange(count + 1, dtype=np.float64) - frac) * ts
    big = np.interp(edges, knots, integral)
    return np.diff(big) / ts


def stream(fs: float, frac: float = 0.0, carrier: float = 0.0, sigma: float = 0.0, frames=None, *, amp: float = 0.5, seed: int = 1,
           lead_us: float = 30.0, gap_us: float = 40.0, start=None):
    """complex64 stream of ``frames`` (default FOUR) -> (z, the sample index at which each frame starts).  ``sigma`` is the
    noise per component against a pulse of 1 (scaled by ``amp`` with the pulse); ``start`` overrides the start indices."""
    frames = FOUR if frames is None else frames
    sps = fs / 1e6
    starts, at = [], int(round(lead_us * sps))
    for k, fr in enumerate(frames):
        starts.append(at if start is None else int(start[k]))
        at = starts[-1] + int(math.ceil((8 + 8 * len(fr) + gap_us) * sps))
    # (a position needs the 120 us of a long frame inside the stream, whatever its own length)
    n = at + int(math.ceil(64 * sps)) if start is None else max(s + int(math.ceil(120 * sps)) + 2 for s in starts)
    env = np.zeros(n, dtype=np.float64)
    for s, fr in zip(starts, frames):
        count = min(int(math.ceil((8 + 8 * len(fr)) * sps)) + 2, n - s)
        env[s : s + count] += pulse_samples(fr, fs, frac, count)
    t = np.arange(n, dtype=np.float64) / fs
    z = amp * env * np.exp(1j * (2.0 * np.pi * carrier * t + 0.3))
    if sigma:
        rng = np.random.default_rng([seed, int(fs), int(frac * 4), int(carrier), int(sigma * 1000)])
        z = z + amp * sigma * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return z.astype(np.complex64), starts


# ---- the stages -----------------------------------------------------------------------------------------------------------


def envelope(z: np.ndarray) -> np.ndarray:
    return np.abs(np.asarray(z, dtype=np.complex64)).astype(np.float32)


def quantise(e: np.ndarray) -> np.ndarray:
    """q = 65535 unless e 65536 < 65535, else rint(e 65536); float32 throughout, half-even.  (A negative e, outside the
    precondition, gives 0.)"""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.asarray(e, dtype=np.float32) * np.float32(65536.0)
        small = x < np.float32(65535.0)
        q = np.where(small, np.rint(np.where(small, np.maximum(x, np.float32(0.0)), np.float32(0.0))), np.float32(65535.0))
    return q.astype(np.uint16)


def chip_plane(q: np.ndarray, h: int) -> np.ndarray:
    """w[i] = sum_{j<h} q[i + j] (int64), i <= N - h."""
    cs = np.concatenate(([0], np.cumsum(np.asarray(q, dtype=np.int64))))
    return cs[h:] - cs[:-h]


def search(q: np.ndarray, pl: dict) -> dict:
    """Every position: flags (uint8), candidates, records [(n, nbits, P, bytes)] sorted by n."""
    q = np.asarray(q)
    n, h, o, span = q.size, pl["h"], pl["o"], pl["span"]
    npos = n - span + 1
    if npos <= 0:
        return dict(flags=np.zeros(0, dtype=np.uint8), candidates=0, records=[])
    w = chip_plane(q, h)

    def chip(k, at=None):
        return w[o[k] : o[k] + npos] if at is None else w[at + o[k]]

    c = [chip(k) for k in range(15)]
    total = c[0] + c[2] + c[7] + c[9]
    ok = (c[0] > c[1]) & (c[2] > c[1]) & (c[2] > c[3]) & (c[7] > c[6]) & (c[7] > c[8]) & (c[9] > c[8]) & (c[9] > c[10])
    for j in (4, 5, 11, 12, 13, 14):
        ok &= 6 * c[j] < total
    at = np.flatnonzero(ok)
    records = []
    if at.size:
        bits = np.stack([chip(16 + 2 * i, at) > chip(17 + 2 * i, at) for i in range(112)], axis=1).astype(np.uint8)
        for row, p in zip(bits, at.tolist()):
            df = int(np.packbits(row[:5])[0]) >> 3
            nbits = 112 if df >= 16 else 56
            data = np.packbits(row[:nbits]).tobytes()
            if df in (11, 17, 18) and syndrome(data) == 0:
                records.append((p, nbits, int(total[p]), data))
    return dict(flags=ok.astype(np.uint8), candidates=int(at.size), records=records)


# ---- the host logic ---------------------------------------------------------------------------------------------------------


def field_of(me: int, first: int, last: int) -> int:
    """Bits first .. last of the 56-bit ME field, counted from 1 at the most significant."""
    return int(format(me, "056b")[first - 1 : last], 2)


def nl(lat: float) -> int:
    lat = abs(lat)
    if lat == 0:
        return 59
    if lat == 87:
        return 2
    if lat > 87:
        return 1
    return int(np.floor(2 * np.pi / np.arccos(1 - (1 - np.cos(np.pi / 30)) / np.cos(lat * np.pi / 180) ** 2)))


def global_position(even, odd, newer_is_odd):
    le, ge, lo, go = even[0] / 2 ** 17, even[1] / 2 ** 17, odd[0] / 2 ** 17, odd[1] / 2 ** 17
    j = math.floor(59 * le - 60 * lo + 0.5)
    lat_e, lat_o = 6.0 * (j % 60 + le), (360.0 / 59.0) * (j % 59 + lo)
    lat_e = lat_e - 360.0 if lat_e >= 270.0 else lat_e
    lat_o = lat_o - 360.0 if lat_o >= 270.0 else lat_o
    if nl(lat_e) != nl(lat_o):
        return None
    z = nl(lat_e)
    m = math.floor(ge * (z - 1) - go * z + 0.5)
    if newer_is_odd:
        lat, lon = lat_o, (360.0 / max(z - 1, 1)) * (m % max(z - 1, 1) + go)
    else:
        lat, lon = lat_e, (360.0 / max(z, 1)) * (m % max(z, 1) + ge)
    return lat, (lon - 360.0 if lon >= 180.0 else lon)


FIELDS = ("time_s", "df", "icao", "raw", "hits", "level", "type_code", "category", "callsign", "altitude_ft", "cpr_odd", "lat_cpr", "lon_cpr",
          "lat", "lon", "speed_kt", "track_deg", "vertical_rate_fpm")


def parse(records: list, pl: dict) -> dict:
    """records [(n, nbits, P, bytes)] -> dict(messages=[dict], aircraft=[dict])."""
    groups = []
    for p, _, level, raw in sorted(records):
        for g in groups:
            if g["raw"] == raw and 0 <= p - g["n"] <= pl["L"]:
                g["hits"] += 1
                break
        else:
            groups.append(dict(n=p, raw=raw, hits=1, P=level))
    messages, latest, craft = [], {}, {}
    for g in groups:
        raw = g["raw"]
        m = dict.fromkeys(FIELDS)
        m.update(time_s=g["n"] / pl["fs"], df=raw[0] >> 3, icao="%06X" % int.from_bytes(raw[1:4], "big"), raw=raw.hex(), hits=g["hits"],
                 level=g["P"] / (4.0 * pl["h"] * 65536.0))
        if m["df"] in (17, 18):
            me = int.from_bytes(raw[4:11], "big")
            tc = m["type_code"] = field_of(me, 1, 5)
            sub = field_of(me, 6, 8)
            if 1 <= tc <= 4:
                m["category"] = sub
                m["callsign"] = "".join(CHARSET[field_of(me, 9 + 6 * k, 14 + 6 * k)] for k in range(8)).replace("_", " ").rstrip()
            elif 9 <= tc <= 18 or 20 <= tc <= 22:
                if tc <= 18:
                    alt = format(field_of(me, 9, 20), "012b")
                    if alt[7] == "1":
                        m["altitude_ft"] = 25 * int(alt[:7] + alt[8:], 2) - 1000
                m["cpr_odd"], m["lat_cpr"], m["lon_cpr"] = field_of(me, 22, 22), field_of(me, 23, 39), field_of(me, 40, 56)
                other = latest.get((m["icao"], 1 - m["cpr_odd"]))
                if other is not None and m["time_s"] - other["time_s"] <= 10.0:
                    even, odd = (other, m) if m["cpr_odd"] else (m, other)
                    fix = global_position((even["lat_cpr"], even["lon_cpr"]), (odd["lat_cpr"], odd["lon_cpr"]), bool(m["cpr_odd"]))
                    if fix is not None:
                        m["lat"], m["lon"] = fix
                latest[(m["icao"], m["cpr_odd"])] = m
            elif tc == 19 and sub in (1, 2):
                mult = 4 if sub == 2 else 1
                v_ew, v_ns, v_r = field_of(me, 15, 24), field_of(me, 26, 35), field_of(me, 38, 46)
                if v_ew and v_ns:
                    vx = mult * (v_ew - 1) * (-1 if field_of(me, 14, 14) else 1)
                    vy = mult * (v_ns - 1) * (-1 if field_of(me, 25, 25) else 1)
                    m["speed_kt"] = math.hypot(vx, vy)
                    m["track_deg"] = math.degrees(math.atan2(vx, vy)) % 360.0
                if v_r:
                    m["vertical_rate_fpm"] = 64 * (v_r - 1) * (-1 if field_of(me, 37, 37) else 1)
        messages.append(m)
        ac = craft.setdefault(m["icao"], dict(icao=m["icao"], callsign=None, lat=None, lon=None, altitude_ft=None, speed_kt=None, track_deg=None,
                                              vertical_rate_fpm=None, messages=0, first_s=m["time_s"], last_s=m["time_s"]))
        ac["messages"] += 1
        ac["last_s"] = m["time_s"]
        for key in ("callsign", "altitude_ft", "speed_kt", "track_deg", "vertical_rate_fpm"):
            if m[key] is not None:
                ac[key] = m[key]
        if m["lat"] is not None:
            ac["lat"], ac["lon"] = m["lat"], m["lon"]
    return dict(messages=messages, aircraft=[craft[k] for k in sorted(craft)])


def oracle(fs: float, q: np.ndarray) -> dict:
    pl = plan(fs)
    out = search(q, pl)
    out.update(parse(out["records"], pl))
    return out


def decode(z: np.ndarray, fs: float) -> dict:
    return oracle(fs, quantise(envelope(z)))


def case_decodes(fs, frac, carrier, sigma):
    """(every kept frame is a transmitted one, all four transmitted frames were kept) for one case of the grid."""
    z, _ = stream(fs, frac, carrier, sigma)
    got = {r[3] for r in decode(z, fs)["records"]}
    return got <= set(FOUR), got == set(FOUR)


# ---- edge shapes (tests/test_gpu_adsb_shapes.py, tests/test_adsb_shapes_host.py) -------------------------------------------
#
# Case tables and numpy stand-ins of the two entry points that follow csrc/adsb.hip's launch arithmetic and can be broken
# one way at a time.  The ``check_*`` functions hold the comparisons; they take the entry point as a callable, so the GPU file
# passes the device call and the host file the stand-in.  ``search`` takes any dict(o, h, span), a plan's or not.

SENT = -7_777_777  # what untouched int64 output words hold
SENT8, SENT16 = 0xAA, 0xAAAA  # ... untouched bytes and halfwords
GUARD = 16  # sentinel elements behind every output
TILE, THREADS = 2048, 256  # IQA_ADSB_TILE, AD_THREADS
MAX_H, MAX_SPAN = 10, 2400
MAX_N = 1 << 40
SLOT_BYTES = 14
HI, LO = 39_000, 1_000
HOSTILE_F32 = np.array([np.nan, np.inf, -np.inf, 3.0e38], dtype=np.float32)
HOSTILE_U16 = np.array([65535, 32768, 65535, 32768], dtype=np.uint16)
HOSTILE_I32 = np.array([2 ** 31 - 1, -(2 ** 31), 2 ** 31 - 1, -(2 ** 31)], dtype=np.int32)
STRICT_PAIRS = ((0, 1), (2, 1), (2, 3), (7, 6), (7, 8), (9, 8), (9, 10))  # (the larger, the smaller) of the seven strict inequalities
QUIET_CHIPS = (4, 5, 11, 12, 13, 14)  # 6 C_j < P


def table(o, h: int, span: int | None = None) -> dict:
    o = np.asarray(o, dtype=np.int64)
    return dict(o=o, h=int(h), span=int(o[-1]) + int(h) if span is None else int(span))


def table_ok(t: dict) -> bool:
    """The ABI's preconditions on an offset table."""
    o = t["o"]
    return o.size == CHIPS and o[0] == 0 and bool((np.diff(o) >= 0).all()) and 1 <= t["h"] <= MAX_H and 1 <= t["span"] <= MAX_SPAN and int(o[-1]) + t["h"] <= t["span"]


def tables() -> dict:
    """The tables that are no plan's, and the plans' at h = 1, 2 and 10."""
    k = np.arange(CHIPS)
    p2, p4, p20 = plan(2e6), plan(4e6), plan(20e6)
    bits = np.unpackbits(np.frombuffer(IDENT, dtype=np.uint8))
    zero, one = int(np.flatnonzero(bits == 0)[7]), int(np.flatnonzero(bits == 1)[7])

    def equal_at(pair_first):
        o = k.copy()
        o[pair_first + 1] = o[pair_first]
        return o

    return {"2 MHz": table(p2["o"], 1), "4 MHz": table(p4["o"], 2), "20 MHz": table(p20["o"], 10), "wide": table(10 * k, 1, 2400), "slack": table(k, 1, 240 + 37),
            "h 3": table(np.rint(3.2 * k), 3), "equal at a 0 bit": table(equal_at(16 + 2 * zero), 1), "equal at a 1 bit": table(equal_at(16 + 2 * one), 1),
            "equal at the preamble": table(equal_at(0), 1)}


def chip_values(h: int, total: int, kind: int = 0) -> np.ndarray:
    """h values that sum to ``total``, pairwise different for h > 1, and different from those of another ``kind``."""
    base = np.full(h, total // h, dtype=np.int64)
    base[0] += total - int(base.sum())
    if h > 1:
        d = np.array([(1 + j // 2 + (h + 1) * kind) * (1 if j % 2 == 0 else -1) for j in range(h - h % 2)], dtype=np.int64)
        base[: d.size] += d
    assert int(base.sum()) == total and (h == 1 or len(set(base.tolist())) == h) and base.min() >= 0 and base.max() <= 65535
    return base


def lay(q: np.ndarray, frame: bytes, t: dict, at: int, hi: int = HI, lo: int = LO, *, chips: int | None = None) -> None:
    """The frame's chips into q from ``at``: every sample of the frame's extent ``lo``, the h samples of a pulsed chip ``hi``
    (the chip at t["o"][k] .. + h)."""
    a = chips_of(frame)
    nchips = a.size if chips is None else chips
    o, h = t["o"], t["h"]
    q[at : at + int(o[nchips - 1]) + h] = lo
    for k in np.flatnonzero(a[:nchips] > 0):
        q[at + int(o[k]) : at + int(o[k]) + h] = hi


def frame_plane(frame: bytes, t: dict, lead: int = 3, tail: int = 5, hi: int = HI, lo: int = LO) -> np.ndarray:
    q = np.full(lead + t["span"] + tail, lo, dtype=np.uint16)
    lay(q, frame, t, lead, hi, lo)
    return q


def period7_plane(n: int) -> np.ndarray:
    """1000, 0, 3000, 0, 0, 0, 0 repeated: at 2 MHz every seventh position passes the preamble rule."""
    return np.resize(np.array([1000, 0, 3000, 0, 0, 0, 0], dtype=np.uint16), n)


def _case(name, t, q, *, keep=(), drop=(), passes=(), misses=(), capacity=8, flags=True, tile0=None, level=None):
    return dict(name=name, table=t, q=np.asarray(q, dtype=np.uint16), keep=list(keep), drop=list(drop), passes=list(passes), misses=list(misses),
                capacity=capacity, flags=flags, tile0=tile0, level=level)


def table_cases() -> list:
    """The search on tables that are no plan's: keep / drop are (position, bytes) the oracle must keep / must not keep."""
    T = tables()
    out = []
    lead = 3
    for name in ("wide", "slack", "h 3"):
        t = T[name]
        second = (1 if lead + t["span"] < TILE else 2) * TILE - 1  # the last position of a tile, behind the first frame
        q = np.full(second + 10 + t["span"], LO, dtype=np.uint16)  # the last tile has 10 positions
        lay(q, IDENT, t, lead)
        lay(q, DF11, t, second)
        out.append(_case(f"table '{name}': o[239] {int(t['o'][-1])} h {t['h']} span {t['span']}", t, q, keep=[(lead, IDENT), (second, DF11)]))
    out.append(_case("table 'slack' on a plane of span - 1 samples: no position", T["slack"], frame_plane(IDENT, T["2 MHz"], 0, 36), drop=[(0, IDENT)]))
    out.append(_case("table 'slack' on a plane of span samples: one position", T["slack"], frame_plane(IDENT, T["2 MHz"], 0, 37), keep=[(0, IDENT)]))
    q = frame_plane(IDENT, T["2 MHz"], lead)
    out.append(_case("equal offsets at a data pair whose bit is 0", T["equal at a 0 bit"], q, keep=[(lead, IDENT)]))
    out.append(_case("equal offsets at a data pair whose bit is 1", T["equal at a 1 bit"], q, drop=[(lead, IDENT)], passes=[lead]))
    out.append(_case("equal offsets at the preamble pair (0, 1)", T["equal at the preamble"], q, drop=[(lead, IDENT)], misses=[lead]))
    return out


def strict_cases(h: int) -> list:
    """h = 2 or 10: for each of the seven strict inequalities and each of the six 6 C_j < P rules a plane where the two sums
    tie although no two samples of the two chips are equal (fails) and one where they differ by 1 (passes); at h = 10 also
    the full-scale pair (pulses of 65 535, P = 2 621 400, a quiet chip of ten samples of 43 690)."""
    t = tables()[{2: "4 MHz", 10: "20 MHz"}[h]]
    o, lead = t["o"], 3
    pulse = 78_000 * h // 2  # a multiple of 3: 6 (2 pulse / 3) = 4 pulse = P
    base = frame_plane(IDENT, t, lead, hi=pulse // h, lo=LO)
    for k in (0, 2, 7, 9):
        base[lead + int(o[k]) : lead + int(o[k]) + h] = chip_values(h, pulse, 0)
    out = []

    def chip(q, k):
        return q[lead + int(o[k]) : lead + int(o[k]) + h]

    for big, small in STRICT_PAIRS:
        for less, passes in ((0, False), (1, True)):
            q = base.copy()
            v = chip_values(h, pulse, 1)
            v[-1] -= less
            chip(q, small)[:] = v
            assert len(set(chip(q, big).tolist()) | set(v.tolist())) == 2 * h and int(chip(q, big).sum()) - int(v.sum()) == less
            out.append(_case(f"h {h}: C{big} against C{small}, {'one less' if less else 'a tie of sums'}", t, q, passes=[lead] if passes else [], misses=[] if passes else [lead],
                             keep=[(lead, IDENT)] if passes else []))
    for j in QUIET_CHIPS:
        for less, passes in ((0, False), (1, True)):
            q = base.copy()
            v = chip_values(h, 4 * pulse // 6, 1)
            v[-1] -= less
            chip(q, j)[:] = v
            assert 6 * int(v.sum()) == 4 * pulse - 6 * less and len(set(v.tolist())) == h
            out.append(_case(f"h {h}: 6 C{j} against P, {'one less' if less else 'equal'}", t, q, passes=[lead] if passes else [], misses=[] if passes else [lead],
                             keep=[(lead, IDENT)] if passes else []))
    if h == 10:
        for less, passes in ((0, False), (1, True)):
            q = frame_plane(IDENT, t, lead, hi=65_535, lo=LO)
            chip(q, 4)[:] = 43_690
            chip(q, 4)[-1] -= less
            assert 6 * 436_900 == 4 * 10 * 65_535 == 2_621_400
            out.append(_case(f"h 10 at full scale: 6 C4 against P = 2 621 400, {'one sample less by 1' if less else 'equal'}", t, q, passes=[lead] if passes else [],
                             misses=[] if passes else [lead], keep=[(lead, IDENT)] if passes else [], level=2_621_400 if passes else None))
    return out


def crowded_cases() -> list:
    """More than 256 passing positions in tile 0: the period-7 plane over three tiles at 2 MHz, alone and with frames laid
    over it inside the last 258 positions of tile 0, one of them across the tile edge."""
    t = tables()["2 MHz"]
    n = 3 * TILE + t["span"] - 1
    out = [_case("period 7 over three tiles", t, period7_plane(n), tile0=293)]
    for name, frames in (("IDENT at 1790", [(1790, IDENT)]), ("POS_EVEN at 1795", [(1795, POS_EVEN)]), ("IDENT across the edge at 2040", [(2040, IDENT)]),
                         ("DF11 at 1900, POS_EVEN across the edge at 2044", [(1900, DF11), (2044, POS_EVEN)])):
        q = period7_plane(n)
        for at, fr in frames:
            lay(q, fr, t, at)
        out.append(_case(f"period 7 with {name}", t, q, keep=frames, tile0=257))
    return out


def register_cases() -> list:
    """``is_long ? reg : reg56`` from both sides, and the DF filter."""
    t = tables()["2 MHz"]
    lead = 3
    out = []
    head17 = bytes([(17 << 3) | 5]) + (0x4840D6).to_bytes(3, "big")
    long_bad = with_parity(head17) + bytes.fromhex("0123456789abcd")
    assert syndrome(long_bad[:7]) == 0 and syndrome(long_bad) != 0
    out.append(_case("a DF17 whose first 56 bits are a codeword and whose 112 are not", t, frame_plane(long_bad, t, lead), drop=[(lead, long_bad)], passes=[lead]))
    short_bad = with_parity(bytes([(11 << 3) | 5]) + bytes.fromhex("4840d6aabbccddeeff0102")[:10])
    assert len(short_bad) == 14 and syndrome(short_bad) == 0 and syndrome(short_bad[:7]) != 0 and short_bad[0] >> 3 == 11
    out.append(_case("a DF11 whose 56 bits fail and whose 112 would pass", t, frame_plane(short_bad, t, lead), drop=[(lead, short_bad), (lead, short_bad[:7])], passes=[lead]))
    for df in (0, 4, 5, 16, 20, 21, 24):
        head = bytes([(df << 3) | 5]) + (0x4840D6).to_bytes(3, "big")
        fr = with_parity(head if df < 16 else head + (0x123456789ABCDE).to_bytes(7, "big"))
        assert syndrome(fr) == 0 and fr[0] >> 3 == df
        out.append(_case(f"a valid DF{df} is dropped", t, frame_plane(fr, t, lead), drop=[(lead, fr)], passes=[lead]))
    for df in (11, 17, 18):
        fr = build_frame(df, 0x40621D, None if df == 11 else 0x58C382D690C8AC)
        q = frame_plane(fr, t, lead)
        if df == 11:  # whatever lies behind a short frame is not read as part of it
            q[lead + 128 :] = np.random.default_rng(3).integers(0, 30_000, size=q.size - (lead + 128)).astype(np.uint16)
        out.append(_case(f"a valid DF{df} is kept", t, q, keep=[(lead, fr)]))
    return out


def optional_cases() -> list:
    """flags_out NULL, and capacity 0 with NULL list and slots, on a plane with three frames; and a list shorter than the
    kept frames."""
    t = tables()["2 MHz"]
    q = np.full(1100, LO, dtype=np.uint16)
    frames = [(5, IDENT), (300, DF11), (600, POS_ODD)]
    for at, fr in frames:
        lay(q, fr, t, at)
    return [_case("three frames, flags NULL", t, q, keep=frames, flags=False), _case("three frames, capacity 0 with NULL list and slots", t, q, keep=frames, capacity=0),
            _case("three frames, capacity 0, flags NULL", t, q, keep=frames, capacity=0, flags=False), _case("three frames, capacity 1", t, q, keep=frames, capacity=1)]


def search_cases() -> list:
    """Every case of the search, each with the uint16 offset of q and the byte offset of flags inside their allocations."""
    out = table_cases() + strict_cases(2) + strict_cases(10) + crowded_cases() + register_cases() + optional_cases()
    for k, case in enumerate(out):
        case["offsets"] = (k % 4, (k // 4 + 3 * k) % 4)
    return out


def check_search(case: dict, call) -> None:
    """``call(q_alloc, q_at, n, o_alloc, o_host, h, span, flags_alloc | None, f_at, list | None, slots | None, capacity,
    counts) -> (flags, list, slots, counts)`` (uint8, int64, uint8, int64 numpy).  The case's own claims are asserted on the
    oracle first."""
    t, q, capacity = case["table"], case["q"], case["capacity"]
    assert table_ok(t), case["name"]
    n, span = q.size, t["span"]
    npos = max(n - span + 1, 0)
    want = search(q, t)
    kept = {(r[0], r[3]) for r in want["records"]}
    assert want["flags"].size == npos and want["candidates"] == int(want["flags"].sum())
    assert all((at, fr) in kept for at, fr in case["keep"]) and not any((at, fr) in kept for at, fr in case["drop"]), case["name"]
    assert all(want["flags"][p] == 1 for p in case["passes"]) and all(want["flags"][p] == 0 for p in case["misses"]), case["name"]
    assert case["keep"] or case["drop"] or case["passes"] or case["misses"] or case["tile0"], case["name"]
    if case["tile0"]:
        assert int(want["flags"][:TILE].sum()) >= case["tile0"] >= 257, case["name"]
    if case["level"]:
        assert [r[2] for r in want["records"] if r[0] == case["keep"][0][0]] == [case["level"]]
    q_off, f_off = case["offsets"]
    q_at, f_at = 8 + q_off, 16 + f_off
    q_alloc = np.concatenate([np.resize(HOSTILE_U16, q_at), q, HOSTILE_U16])
    o_host = np.ascontiguousarray(t["o"], dtype=np.int32)
    o_alloc = np.concatenate([o_host, HOSTILE_I32])
    flags = np.full(f_at + npos + GUARD, SENT8, dtype=np.uint8) if case["flags"] else None
    lst = np.full(3 * capacity + GUARD, SENT, dtype=np.int64) if capacity else None
    slots = np.full(SLOT_BYTES * capacity + GUARD, SENT8, dtype=np.uint8) if capacity else None
    beside = [np.full(GUARD, SENT, dtype=np.int64) for _ in range(2)]  # what capacity 0 could have written into
    counts = np.array([99, 99, SENT, SENT], dtype=np.int64)
    flags, lst, slots, counts = call(q_alloc, q_at, n, o_alloc, o_host, t["h"], span, flags, f_at, lst, slots, capacity, counts)
    assert [int(v) for v in counts] == [len(want["records"]), want["candidates"], SENT, SENT], case["name"]
    assert all((b == SENT).all() for b in beside)
    if case["flags"]:
        np.testing.assert_array_equal(flags[f_at : f_at + npos], want["flags"], err_msg=case["name"])
        assert (flags[:f_at] == SENT8).all() and (flags[f_at + npos :] == SENT8).all(), case["name"]
    if not capacity:
        return
    k = min(len(want["records"]), capacity)
    entries, data = lst[: 3 * capacity].reshape(-1, 3), slots[: SLOT_BYTES * capacity].reshape(capacity, SLOT_BYTES)
    assert (entries[k:] == SENT).all() and (lst[3 * capacity :] == SENT).all() and (data[k:] == SENT8).all() and (slots[SLOT_BYTES * capacity :] == SENT8).all()
    got = sorted((int(e[0]), int(e[1]), int(e[2]), data[i].tobytes()) for i, e in enumerate(entries[:k]))
    full = [(p, nb, lv, raw.ljust(SLOT_BYTES, b"\0")) for p, nb, lv, raw in want["records"]]
    assert got == full if len(full) <= capacity else all(g in full for g in got), case["name"]


def kernel_search(q, n: int, o, h: int, span: int, flags, lst, slots, capacity: int, counts, *, one_round: bool = False, reg_for_short: bool = False,
                  le_rule: int | None = None) -> None:
    """k_adsb_search and its launch in numpy, tile by tile: the staged samples (zero behind the stream), the chip-sum plane w,
    pass 1 over the live positions (a thread's positions are tid + 256 r, so the list in LDS is modelled in ascending
    position order), pass 2 over that list in rounds of 256 with the 24-bit register run over all 112 bits and read out
    behind bit 55.  Breaks: ``one_round`` stops pass 2 after its first round; ``reg_for_short`` tests the 112-bit register for
    a short frame too; ``le_rule`` = j turns 6 C_j < P into <=."""
    o = np.asarray(o[:CHIPS], dtype=np.int64)
    npos = n - span + 1
    at_list = 0
    for b in range(-(-npos // TILE)):
        t0 = b * TILE
        nw, nq = TILE + span - h, TILE + span
        s_q = np.zeros(nq, dtype=np.int64)
        m = min(nq, n - t0)
        s_q[:m] = q[t0 : t0 + m]
        cs = np.concatenate(([0], np.cumsum(s_q)))
        s_w = (cs[h:] - cs[:-h])[:nw]
        live = min(npos - t0, TILE)
        i = np.arange(live)
        c = [s_w[i + o[k]] for k in range(15)]
        P = c[0] + c[2] + c[7] + c[9]
        ok = (c[0] > c[1]) & (c[2] > c[1]) & (c[2] > c[3]) & (c[7] > c[6]) & (c[7] > c[8]) & (c[9] > c[8]) & (c[9] > c[10])
        for j in QUIET_CHIPS:
            ok &= (6 * c[j] <= P) if le_rule == j else (6 * c[j] < P)
        if flags is not None:
            flags[t0 : t0 + live] = ok
        s_list = np.flatnonzero(ok)
        if not s_list.size:
            continue
        counts[1] += s_list.size
        for r0 in range(0, s_list.size, THREADS):
            if one_round and r0:
                break
            for p in s_list[r0 : r0 + THREADS].tolist():
                reg = reg56 = 0
                bits = (s_w[p + o[16::2]] > s_w[p + o[17::2]]).astype(np.uint8)
                for k, bit in enumerate(bits.tolist()):
                    reg = (reg << 1) | bit
                    if reg & 0x1000000:
                        reg ^= GENERATOR
                    if k == 55:
                        reg56 = reg
                df = int(np.packbits(bits[:5])[0]) >> 3
                is_long = df >= 16
                if df not in (11, 17, 18) or (reg if (is_long or reg_for_short) else reg56) != 0:
                    continue
                counts[0] += 1
                if at_list >= capacity:
                    continue
                nbits = 112 if is_long else 56
                lst[3 * at_list : 3 * at_list + 3] = (t0 + p, nbits, int(P[p]))
                slots[SLOT_BYTES * at_list : SLOT_BYTES * (at_list + 1)] = np.frombuffer(np.packbits(bits[:nbits]).tobytes().ljust(SLOT_BYTES, b"\0"), dtype=np.uint8)
                at_list += 1


def entry_search(q_alloc, q_at, n, o_alloc, o_host, h, span, flags, f_at, lst, slots, capacity, counts, **breaks):
    """iqa_adsb_search's checks in front of ``kernel_search``; None stands for a NULL pointer."""
    if n < 0 or capacity < 0:
        raise ValueError("negative length")
    if counts is None:
        raise ValueError("NULL device pointer")
    if o_host is None:
        raise ValueError("NULL offset table")
    if not 1 <= h <= MAX_H:
        raise ValueError("h must be 1 .. IQA_ADSB_MAX_SPS / 2")
    if not 1 <= span <= MAX_SPAN:
        raise ValueError("span must be 1 .. IQA_ADSB_MAX_SPAN")
    if o_host[0] != 0:
        raise ValueError("o[0] must be 0")
    if (np.diff(np.asarray(o_host[:CHIPS], dtype=np.int64)) < 0).any():
        raise ValueError("the offsets must ascend")
    if int(o_host[CHIPS - 1]) + h > span:
        raise ValueError("o[239] + h must be <= span")
    if n > MAX_N:
        raise ValueError("length out of range")
    if n >= span and (q_alloc is None or o_alloc is None or (capacity > 0 and (lst is None or slots is None))):
        raise ValueError("NULL device pointer")
    counts[:2] = 0
    if n >= span:
        kernel_search(q_alloc[q_at:], n, o_alloc, h, span, None if flags is None else flags[f_at:], lst, slots, capacity, counts, **breaks)
    return flags, lst, slots, counts


def search_refusals() -> list:
    """(what, n, o_host | None, h, span, capacity, q?, o_dev?, list?, slots?, counts?, message)."""
    o = np.arange(CHIPS, dtype=np.int32)
    yes = (True,) * 5

    def bent(k, v):
        out = o.copy()
        out[k] = v
        return out

    return [("negative n", -1, o, 1, 240, 4) + yes + ("negative",), ("negative capacity", 500, o, 1, 240, -1) + yes + ("negative",),
            ("NULL counts", 500, o, 1, 240, 4, True, True, True, True, False, "NULL"), ("NULL offset table", 500, None, 1, 240, 4) + yes + ("NULL offset table",),
            ("h 0", 500, o, 0, 240, 4) + yes + ("h must be",), ("h 11", 500, o, 11, 260, 4) + yes + ("h must be",),
            ("span 0", 500, o, 1, 0, 4) + yes + ("span must be",), ("span 2401", 2500, o, 1, 2401, 4) + yes + ("span must be",),
            ("o[0] not 0", 500, bent(0, 1), 1, 240, 4) + yes + (r"o\[0\] must be 0",), ("a descending pair", 500, bent(100, 98), 1, 240, 4) + yes + ("must ascend",),
            ("o[239] + h above span", 500, o, 2, 240, 4) + yes + (r"o\[239\] \+ h",), ("n above 2^40", MAX_N + 1, o, 1, 240, 4) + yes + ("out of range",),
            ("NULL q", 500, o, 1, 240, 4, False, True, True, True, True, "NULL"), ("NULL offsets", 500, o, 1, 240, 4, True, False, True, True, True, "NULL"),
            ("NULL list", 500, o, 1, 240, 4, True, True, False, True, True, "NULL"), ("NULL slots", 500, o, 1, 240, 4, True, True, True, False, True, "NULL")]


# -- the quantiser


QUANTISE_LENGTHS = (0, 1, 255, 256, 257, 2049)
QUANTISE_VALUES = np.concatenate([
    np.array([np.nan, np.inf, 3.0e38, 1.0, 65535.0 / 65536.0, 65534.5 / 65536.0, 65533.5 / 65536.0, 0.5, 2.0 ** -17, 1.5 * 2.0 ** -16, 2.5 * 2.0 ** -16, 0.0,
              2.0 ** -140, -0.0, -1.0, -np.inf]),
    (np.arange(0, 12) + 0.5) / 65536.0, (np.arange(32760, 32772) + 0.5) / 65536.0]).astype(np.float32)
QUANTISE_WANT = [65535, 65535, 65535, 65535, 65535, 65534, 65534, 32768, 0, 2, 2, 0, 0, 0, 0, 0] + [0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12] + [
    32760, 32762, 32762, 32764, 32764, 32766, 32766, 32768, 32768, 32770, 32770, 32772]


def quantise_cases() -> list:
    """dict(name, n, e, offsets): the value list at the front of every plane that holds it, random values in 0 .. 1.2 behind
    it; ``e`` and ``q_out`` views at odd element offsets."""
    out = []
    for k, n in enumerate(QUANTISE_LENGTHS):
        e = np.random.default_rng(n).uniform(0.0, 1.2, n).astype(np.float32)
        m = min(n, QUANTISE_VALUES.size)
        e[:m] = QUANTISE_VALUES[:m]
        if n > QUANTISE_VALUES.size:
            e[-1] = np.float32(np.nan)
        out.append(dict(name=f"n {n}", n=n, e=e, offsets=((1, 3), (3, 1), (1, 1), (3, 3), (1, 3), (3, 1))[k]))
    return out


def check_quantise(case: dict, call) -> None:
    """``call(e_alloc, e_at, n, q_alloc, q_at) -> q_alloc`` (uint16 numpy)."""
    n, e = case["n"], case["e"]
    want = quantise(e)
    assert want[: QUANTISE_VALUES.size].tolist() == QUANTISE_WANT[:n]
    e_at, q_at = 4 + case["offsets"][0], 8 + case["offsets"][1]
    e_alloc = np.concatenate([np.resize(np.array([0.25, 0.75], dtype=np.float32), e_at), e, np.array([0.25, 0.75, 0.25, 0.75], dtype=np.float32)])
    q_alloc = call(e_alloc, e_at, n, np.full(q_at + n + GUARD, SENT16, dtype=np.uint16), q_at)
    np.testing.assert_array_equal(q_alloc[q_at : q_at + n], want, err_msg=case["name"])
    assert (q_alloc[:q_at] == SENT16).all() and (q_alloc[q_at + n :] == SENT16).all(), case["name"]


def entry_quantise(e_alloc, e_at, n, q_alloc, q_at):
    if n < 0:
        raise ValueError("negative length")
    if n == 0:
        return q_alloc
    if e_alloc is None or q_alloc is None:
        raise ValueError("NULL device pointer")
    if n > MAX_N:
        raise ValueError("length out of range")
    q_alloc[q_at : q_at + n] = quantise(e_alloc[e_at : e_at + n])
    return q_alloc


def quantise_refusals() -> list:
    """(what, n, e?, q?, message)."""
    return [("negative n", -1, True, True, "negative"), ("NULL e", 64, False, True, "NULL"), ("NULL q_out", 64, True, False, "NULL"),
            ("n above 2^40", MAX_N + 1, True, True, "out of range")]
