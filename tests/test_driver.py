"""shud_rhs.driver's device-free part: the reference's setSink rule (MD_initialize.cpp:348-356), which print control
gets which NetCDF file."""
from shud_rhs.driver import sink_kind


def test_sink_kind_restates_set_sink():
    for mode in (1, 2):                                  # NETCDF, BOTH
        assert sink_kind(2000, 2000, 300, 4, mode) == "ele"
        assert sink_kind(300, 2000, 300, 4, mode) == "riv"
        assert sink_kind(4, 2000, 300, 4, mode) == "lake"
        assert sink_kind(7, 7, 7, 7, mode) == "ele"      # NumEle == NumRiv: the element sink wins
        assert sink_kind(7, 9, 7, 7, mode) == "riv"      # NumRiv == NumLake: reaches come before lakes
        assert sink_kind(0, 2000, 0, 0, mode) is None    # no reaches: a control of 0 columns is not a river one
        assert sink_kind(0, 2000, 300, 0, mode) is None  # no lakes: nor a lake one
        assert sink_kind(0, 0, 0, 0, mode) == "ele"      # the element file exists whatever NumEle is
        assert sink_kind(5, 2000, 300, 4, mode) is None  # NumAll matches nothing
    for n_all in (2000, 300, 4, 5, 0):                   # LEGACY: never a sink
        assert sink_kind(n_all, 2000, 300, 4, 0) is None
