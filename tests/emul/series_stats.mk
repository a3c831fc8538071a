# TEST-ONLY host build of the series walk with per-bin statistics (three planes per row and partial slot, the fix-up's
# plane dimension) over rtl-power-fftw_amd/csrc/series_partition.h: series_stats_emul.cpp -> librpf_emul_series_stats.so,
# loaded by tests/test_series_stats.py.  A makefile of its own (make -f series_stats.mk), as series.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_series_stats.so: series_stats_emul.cpp $(CSRC)/series_partition.h $(CSRC)/hop_partition.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ series_stats_emul.cpp
clean:
	rm -f librpf_emul_series_stats.so
.PHONY: clean
