"""Golden vectors of the reference's stellar-spectrum binning (build container only).

    PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 -W ignore tests/golden/make_stellar_goldens.py

Runs the reference's own ``frei.phoenix.get_binned_phoenix_spectrum`` (phoenix.py:20-52, with
``resolution``, phoenix.py:13-17) unmodified.  Stand-ins:

* ``frei.phoenix.get_spectrum`` (the ``expecto`` download, phoenix.py:42) is a stub that
  returns seeded arrays as Quantities, wavelengths in µm so ``.to(u.um)`` is the identity;
* ``xarray.DataArray`` is ``binharness.XArr`` (``integrate``: duck_array_ops.trapz,
  ``expand_dims``, coordinate ``max``/``min``/``mean``) plus ``groupby_bins``: the real
  ``pandas.cut`` codes (right-closed bins), empty groups dropped, ``map`` over the groups in bin
  order and concatenation along the dimension.

Writes ``stellar_bin.npz`` (inputs + outputs, no pickles): about 4.9 k points on a
piecewise-constant axis, 3 spectra and two grids — ``a`` with every bin filled, ``b`` whose
leading bins lie below the spectrum and whose fine bins hold 0, 1 or 2 points (NaN for the
single-point ones, a shifted and zero-padded result).
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import binharness as BH  # noqa: E402

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import astropy.units as u  # noqa: E402

R = BH.load()


class _Groups:
    def __init__(self, arr, dim, bins):
        self.arr, self.dim = arr, dim
        codes = pd.cut(np.asarray(arr.coords[dim]), np.asarray(bins)).codes
        self.groups = [np.nonzero(codes == c)[0] for c in np.unique(codes[codes >= 0])]

    def map(self, func, **kwargs):
        parts = [func(self.arr.isel(self.dim, idx), **kwargs) for idx in self.groups]
        return BH._concat(parts, self.dim)


class SpecArr(BH.XArr):
    """binharness.XArr with the keyword constructor phoenix.py:43-46 uses and groupby_bins."""

    def __init__(self, data, dims=None, coords=None, name=None):
        super().__init__(data, dims, {k: np.asarray(v) for k, v in (coords or {}).items()}, name)

    def groupby_bins(self, dim, bins):
        return _Groups(self, dim, bins)


def axis():
    """Piecewise-constant spacing, like a PHOENIX axis: 0.3-1 µm at 5e-4, 1-2.5 at 1e-3,
    2.5-5.5 at 1.5e-3."""
    return np.concatenate([0.3 + 5e-4 * np.arange(1400), 1.0 + 1e-3 * np.arange(1500),
                           2.5 + 1.5e-3 * np.arange(2000)])


def spectra(wl, rng):
    out = []
    for T in (3000.0, 4500.0, 6000.0):
        x = 1.4388e4 / (wl * T)
        planck = 1e15 * wl ** -5 / np.expm1(x)
        out.append(planck * rng.lognormal(0.0, 0.5, wl.size))
    return np.array(out)


def edges(lam):
    d0 = lam[1] - lam[0]
    return np.concatenate([[lam.min() - d0], lam]) + d0 / 2      # core.py:34-45


def main():
    import importlib
    phoenix = importlib.import_module("frei.phoenix")
    sys.modules["xarray"].DataArray = SpecArr
    flux_unit = R.twostream.flux_unit
    rng = np.random.default_rng(20)
    wl = axis()
    flux = spectra(wl, rng)
    assert np.all(np.diff(wl) > 0) and np.all(flux > 0)
    out = dict(wl=wl, flux=flux)
    grids = dict(a=np.logspace(np.log10(0.5), np.log10(5.0), 60),
                 b=np.logspace(np.log10(0.25), np.log10(3.0), 2500))
    for name, lam in grids.items():
        wl_bins = edges(lam)
        res = []
        for m in range(flux.shape[0]):
            phoenix.get_spectrum = lambda T, log_g=None, cache=True, m=m: types.SimpleNamespace(
                wavelength=wl * u.um, flux=flux[m] * flux_unit)
            r = phoenix.get_binned_phoenix_spectrum(4000 * u.K, 1e4 * u.cm / u.s ** 2, wl_bins,
                                                    lam * u.um)
            assert r.unit == flux_unit and r.shape == lam.shape
            res.append(r.value)
        res = np.array(res)
        out[f"{name}_lam"], out[f"{name}_wl_bins"], out[f"{name}_out"] = lam, wl_bins, res
        print(name, res.shape, "nan:", int(np.isnan(res[0]).sum()), "zero-padded:",
              int((res[0] == 0).sum()))
    dest = os.path.join(HERE, "stellar_bin.npz")
    np.savez_compressed(dest, **out)
    print(f"wrote stellar_bin.npz: {os.path.getsize(dest) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
