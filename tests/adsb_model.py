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
