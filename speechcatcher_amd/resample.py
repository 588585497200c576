"""Host arithmetic of the sample-rate conversion (the kernel and the filter design are csrc/resample.hip):
which input rates the engine takes and how many 16 kHz samples a stream has produced after N input samples - integer
formulas the host layers use to keep their clocks in 16 kHz samples without asking the device."""
import math

OUTPUT_RATE = 16000
MIN_RATE, MAX_RATE, MAX_PHASES = 8000, 48000, 640
COMMON_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)


def rate_params(rate: int):
    """-> (L, M, half width Wc) of the design for ``rate``, None for an unsupported rate"""
    if not MIN_RATE <= rate <= MAX_RATE:
        return None
    g = math.gcd(rate, OUTPUT_RATE)
    L, M = OUTPUT_RATE // g, rate // g
    if L > MAX_PHASES:
        return None
    return L, M, int(math.ceil(24.0 / (0.94 * min(1.0, L / M))))


def check_input_rate(rate) -> int:
    """the rate as an int; ValueError (naming what is supported) for anything the engine does not convert"""
    try:
        r = int(rate)
        whole = float(rate) == r
    except (TypeError, ValueError):
        r, whole = -1, False
    if not whole or rate_params(r) is None:
        raise ValueError(f"unsupported sample rate {rate!r}: the engine takes {MIN_RATE}..{MAX_RATE} Hz with "
                         f"{OUTPUT_RATE} / gcd(rate, {OUTPUT_RATE}) <= {MAX_PHASES} "
                         f"({', '.join(str(r) for r in COMMON_RATES)} among them)")
    return r


def out_count(rate: int, n_in_total: int, final: bool) -> int:
    """16 kHz samples a stream at ``rate`` has produced after ``n_in_total`` input samples (final: after the flush)"""
    if rate == OUTPUT_RATE:
        return n_in_total
    L, M, Wc = rate_params(rate)
    n = n_in_total if final else n_in_total - Wc
    return 0 if n <= 0 else -((-n * L) // M)


class OutputClock:
    """16 kHz samples of every call of one stream at ``rate``: ``call(n_in, final)`` -> samples the call appended"""

    def __init__(self, rate: int = OUTPUT_RATE):
        self.rate, self.n_in, self.n_out = rate, 0, 0
        self.fed = False          # a call has been made

    def call(self, n_in: int, final: bool) -> int:
        self.fed = True
        self.n_in += int(n_in)
        total = out_count(self.rate, self.n_in, final)
        n = total - self.n_out
        self.n_out = total
        if final:
            self.n_in = self.n_out = 0
        return n
