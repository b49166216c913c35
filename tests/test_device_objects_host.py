"""Host-side tests of what the device-side objects share (frei_amd/_device.py): where a call's
spectra come from, as Instrument.apply, CrossCorrelator.correlate and Broadening.apply refuse a
wrong source before any device work, and the timing and release bookkeeping of the four classes.
No GPU: no device handle is ever created."""
import numpy as np
import pytest

N_LAM = 50


def _lam():
    return np.logspace(np.log10(0.5), 1.0, N_LAM)


def _instrument():
    import frei_amd as fa
    return fa.Instrument.top_hat(_lam(), [1.0], [2.0])


def _correlator():
    import frei_amd as fa
    lam = _lam()
    return fa.CrossCorrelator(lam, lam[10:40], np.ones(30), [-5.0, 0.0, 5.0])


def _broadening():
    import frei_amd as fa
    return fa.Broadening(_lam(), fa.BroadeningKernel.gaussian(resolving_power=20.0))


def _stellar():
    import frei_amd as fa
    return fa.StellarSpectra(_lam(), np.ones(N_LAM))


CONSUMERS = {"instrument": (_instrument, "apply"), "correlator": (_correlator, "correlate"),
             "broadening": (_broadening, "apply")}


class SliceEngine:            # an engine on a slice of the axis; any other use is an AttributeError
    n_lam = N_LAM // 2
    lam_um = np.ones(N_LAM)


def _stale():
    from frei_amd.broaden import BroadenedSpectra
    owner = _broadening()
    kept = BroadenedSpectra(owner, owner._serial, 1, True)
    owner._serial += 1        # as the owner's next apply or release does
    return kept


SOURCES = {
    "wrong last dimension": (lambda: dict(x=np.ones(N_LAM + 1)), ValueError, "n_lam"),
    "wrong last dimension, batched": (lambda: dict(x=np.ones((2, N_LAM - 1))), ValueError,
                                      "n_lam"),
    "three dimensions": (lambda: dict(x=np.ones((2, 2, N_LAM))), ValueError, "n_lam"),
    "neither x nor engine": (lambda: dict(x=None), ValueError, "engine"),
    "slice engine": (lambda: dict(x=None, engine=SliceEngine()), ValueError, "slice"),
    "stale kept spectra": (lambda: dict(x=_stale()), RuntimeError, "stale"),
}


# kept spectra feed the two consumers, not a second broadening
CASES = [(c, s) for c in CONSUMERS for s in SOURCES
         if not (c == "broadening" and s == "stale kept spectra")]


@pytest.mark.parametrize("consumer, source", CASES)
def test_a_wrong_source_is_refused_before_any_device_work(consumer, source):
    make, method = CONSUMERS[consumer]
    obj = make()
    kwargs, error, message = SOURCES[source]
    with pytest.raises(error, match=message):
        getattr(obj, method)(**kwargs())
    assert obj._handle is None


@pytest.mark.parametrize("make", [_stellar, _instrument, _correlator, _broadening],
                         ids=["StellarSpectra", "Instrument", "CrossCorrelator", "Broadening"])
def test_timing_accumulates_and_resets_and_release_twice_is_harmless(make):
    obj = make()
    assert obj.timing() == (0.0, 0) and obj.form_used is None
    obj._ms, obj._calls = 1.5, 3          # as three calls would leave them
    assert obj.timing() == (1.5, 3)
    assert obj.timing(reset=True) == (1.5, 3)
    assert obj.timing() == (0.0, 0)
    obj.release()
    obj.release()
    assert obj._handle is None
