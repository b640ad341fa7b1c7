"""gflow_amd.companion without a device: when the second engine is replaced and what it is primed with (stub engines)."""
from types import SimpleNamespace

import pytest
import torch

from gflow_amd.companion import SecondEngine, fits


class StubEngine:
    def __init__(self, cap, K_cap=4_000_000, N=0):
        self.cap, self.K_cap, self.N = cap, K_cap, N
        self.pose, self.intr = torch.zeros(7), torch.zeros(4)
        self.hp = SimpleNamespace(bg=0.0)

    def set_count(self, n):
        assert n <= self.cap
        self.N = n


def test_fits_asks_for_rows_and_optionally_for_pairs():
    assert not fits(None, 0) and not fits(None, 0, 1)
    eng = StubEngine(cap=2048, K_cap=1000)
    assert fits(eng, 2048) and not fits(eng, 2049)
    assert fits(eng, 10, 1000) and not fits(eng, 10, 1001) and not fits(eng, 2049, 10)
    assert fits(eng, 10, None)


@pytest.mark.parametrize("cap,n,made", [(2048, 1500, [2048]),          # first use: max(main.cap, main.N)
                                        (2048, 2048, [2048]),          # exactly full: fits
                                        (4096, 2250, [4096])])
def test_follow_makes_an_engine_on_first_use_with_the_main_engines_room(cap, n, made):
    calls = []
    second = SecondEngine(lambda capacity, K_cap=None: calls.append((capacity, K_cap)) or StubEngine(capacity))
    assert second.engine is None
    main = StubEngine(cap, N=n)
    assert second.follow(main, 0.33) is second.engine
    assert calls == [(c, None) for c in made]


def test_follow_replaces_the_engine_exactly_when_the_rows_no_longer_fit_and_primes_it():
    calls = []
    second = SecondEngine(lambda capacity, K_cap=None: calls.append(capacity) or StubEngine(capacity))
    main = StubEngine(2048, N=1500)
    main.pose, main.intr = torch.arange(7.0), torch.arange(4.0) + 10
    first = second.follow(main, 1.0)
    assert calls == [2048]
    for n in (1, 2048, 1500):                        # fewer rows, as many as fit: the same engine
        main.N = n
        assert second.follow(main, 1.0) is first and first.N == n
    assert calls == [2048]
    main.cap, main.N = 4096, 2250                    # the main engine grew: cap < main.N
    main.pose, main.intr = main.pose + 1, main.intr * 2
    grown = second.follow(main, 0.33)
    assert calls == [2048, 4096] and grown is second.engine and grown is not first and grown.cap == 4096
    assert grown.N == 2250 and grown.hp.bg == 0.33
    assert torch.equal(grown.pose, main.pose) and torch.equal(grown.intr, main.intr)
    assert grown.pose is not main.pose and grown.intr is not main.intr            # (copies, not the main engine's tensors)
    main.N, main.cap = 5000, 4096                    # rows appended beyond the main engine's own room: max(cap, N)
    assert second.follow(main, 0.0).cap == 5000 and calls == [2048, 4096, 5000]
