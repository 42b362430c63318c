# builds the C++ harness of the proof of work (pow_test.cpp -> libpowtest.so) with the host compiler:
#   make -C tests/cpp -f pow.mk
ROOT := ../..
SHIM_HDR := $(wildcard $(ROOT)/crypto3-zk_amd/include/nil/crypto3/zk/hip/*.hpp) $(ROOT)/include/zkhip.h
libpowtest.so: pow_test.cpp $(SHIM_HDR) $(ROOT)/crypto3-zk_amd/libzkhip.so
	g++ -std=c++17 -O2 -fPIC -pthread -shared -I $(ROOT)/crypto3-zk_amd/include -I $(ROOT)/include pow_test.cpp -L $(ROOT)/crypto3-zk_amd -lzkhip -Wl,-rpath,'$$ORIGIN/../../crypto3-zk_amd' -o $@
