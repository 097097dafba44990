# tests/host/zstd_batch_host.mk -- TEST INFRASTRUCTURE ONLY: the batched zstd encoder through the C ABI (zstd_batch_host.cpp) against the AddressSanitizer build of
# the emulator library, run with leak detection on -- the counterpart of `make -C tests/emu lifecycle`:
#     make -C tests/host -f zstd_batch_host.mk          builds tests/emu/_asan/libgpucodec_asan.so (tests/emu/Makefile, target asan), the program beside it, and runs it
# CPU only: nothing here opens a GPU.
EMU = ../emu
ASAN = $(EMU)/_asan

zstd_batch_host: $(ASAN)/zstd_batch_host
	ASAN_OPTIONS=detect_leaks=1 $(ASAN)/zstd_batch_host

$(ASAN)/libgpucodec_asan.so: FORCE
	$(MAKE) -C $(EMU) asan

$(ASAN)/zstd_batch_host: zstd_batch_host.cpp $(ASAN)/libgpucodec_asan.so
	g++ -O1 -g -std=c++17 -fsanitize=address -fno-omit-frame-pointer -I../../include zstd_batch_host.cpp -o $@ -L$(ASAN) -lgpucodec_asan -Wl,-rpath,'$$ORIGIN'

FORCE:
.PHONY: zstd_batch_host FORCE
