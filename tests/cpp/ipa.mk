# builds the harness of the inner-product-argument commitment:  make -C tests/cpp -f ipa.mk
#   libipatest.so  kimchi_pedersen_hip over pallas / vesta (ipa_test.cpp, host compiler)
ROOT := ../..
SHIM_HDR := $(wildcard $(ROOT)/crypto3-zk_amd/include/nil/crypto3/zk/hip/*.hpp) $(ROOT)/include/zkhip.h
all: libipatest.so
libipatest.so: ipa_test.cpp $(SHIM_HDR) $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp) $(ROOT)/crypto3-zk_amd/libzkhip.so
	g++ -std=c++17 -O2 -fPIC -pthread -shared -I $(ROOT)/crypto3-zk_amd/include -I $(ROOT)/include ipa_test.cpp -L $(ROOT)/crypto3-zk_amd -lzkhip -Wl,-rpath,'$$ORIGIN/../../crypto3-zk_amd' -o $@
