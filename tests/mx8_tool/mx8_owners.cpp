// mx8_owners.cpp -- data owners that replay archive files over several rounds, for the end-to-end test of
// fa_aggregator --mx8 (a multi-round sibling of tests/replay_tool: the tool never looks inside an archive, so a
// round's file may be a full model part or an MX8 receipt).
//
//   fa_mx8_owners --dir DIR --out OUT -d D -c C --parts 1,2,3 --rounds R --port-base P [--reply-timeout SECONDS]
//
// The refactor frame once, then R rounds of the protocol (data_owner.cpp:96-112, :225-253): in round r = 1 .. R
// owner k (ids 0, C+1, ..., C+D-1, in that order) sends DIR/r<r>/mp1_owner<k>.pt and, once every owner has its
// reply, the other parts.  Every reply archive is written as it arrives, to OUT/r<r>_reply_mp<part>_port<port>_<i>.pt:
// the i-th reply of round r for that part on that owner port (owners 2 and 3 share a port).  Nothing is checked here:
// the test reads the files.  Exit 0 when every reply came, 1 on a timeout or a failed send.
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "net.h"
#include "wire.h"

using namespace fahost;

namespace {

long now_ms() {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch())
        .count();
}

std::string slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

}  // namespace

int main(int argc, char** argv) {
    std::string dir, out;
    std::vector<int> parts;
    int D = 1, C = 1, port_base = 8079, rounds = 1;
    double reply_timeout_s = 60;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string a = argv[i], v = argv[i + 1];
        if (a == "--dir") dir = v;
        else if (a == "--out") out = v;
        else if (a == "-d") D = std::atoi(v.c_str());
        else if (a == "-c") C = std::atoi(v.c_str());
        else if (a == "--rounds") rounds = std::atoi(v.c_str());
        else if (a == "--port-base") port_base = std::atoi(v.c_str());
        else if (a == "--reply-timeout") reply_timeout_s = std::atof(v.c_str());
        else if (a == "--parts") {
            std::stringstream ss(v);
            std::string t;
            while (std::getline(ss, t, ',')) parts.push_back(std::atoi(t.c_str()));
        } else {
            std::cerr << "unknown argument " << a << "\n";
            return 2;
        }
    }
    if (dir.empty() || out.empty() || parts.empty() || D < 1 || rounds < 1) {
        std::cerr << "usage: fa_mx8_owners --dir DIR --out OUT -d D -c C --parts 1,2,3 --rounds R --port-base P\n";
        return 2;
    }
    std::vector<int> ids = {0};
    for (int i = 0; i < D - 1; ++i) ids.push_back(i + C + 1);
    RoutingTable routes(port_base);
    std::map<int, std::unique_ptr<NetLayer>> listeners;  // owner port -> its listener
    for (int id : ids) {
        const int port = routes.port_for(id);
        if (listeners.count(port)) continue;
        auto nl = std::make_unique<NetLayer>(id, routes);
        if (!nl->start(port)) {
            std::cerr << "cannot listen on " << port << "\n";
            return 1;
        }
        listeners[port] = std::move(nl);
    }
    auto send_to_aggregator = [&](const Bytes& f) {
        const int fd = connect_to(routes.host_for(-1), routes.port_for(-1), 100, 100);
        const bool ok = fd >= 0 && send_all(fd, f.data(), f.size());
        if (fd >= 0) close(fd);
        return ok;
    };
    Message rf;  // the init node's refactor message, once
    rf.type = REFACTOR_DATA_OWNER;
    rf.model_name = 1;
    rf.model_type = 0;
    rf.start = 9;
    rf.end = 3;
    rf.num_classes = 10;
    rf.dataset = 0;
    rf.data_owners = ids;
    rf.read_table = 0;
    int replies = 0;
    bool ok = send_to_aggregator(*frame_bytes(rf));
    for (int round = 1; round <= rounds && ok; ++round) {
        std::map<std::pair<int, int>, int> seen;  // (part, port) -> replies so far this round
        for (int phase = 1; phase <= 2 && ok; ++phase) {
            int want = 0;  // one reply per bucket of the phase and owner
            for (int mp : parts)
                if ((phase == 1) == (mp == 1)) want += D;
            for (int k = 0; k < D && ok; ++k)
                for (int mp : parts) {
                    if ((phase == 1) != (mp == 1)) continue;
                    const std::string blob = slurp(dir + "/r" + std::to_string(round) + "/mp" + std::to_string(mp) +
                                                   "_owner" + std::to_string(k) + ".pt");
                    if (blob.empty()) {
                        std::cerr << "no archive for part " << mp << " of owner " << k << " in round " << round << "\n";
                        return 2;
                    }
                    Message m;  // Task(myID, aggregation_, -1), data_owner.cpp:225-231
                    m.type = OPERATION;
                    m.client_id = ids[(size_t)k];
                    m.prev_node = -1;
                    m.type_op = AGGREGATION;
                    m.model_part = mp;
                    m.t_start = now_ms();
                    char* vals = nullptr;
                    auto f = operation_frame(m, blob.size(), &vals);
                    std::memcpy(vals, blob.data(), blob.size());
                    ok = ok && send_to_aggregator(*f);
                }
            const long t_end = now_ms() + (long)(reply_timeout_s * 1000);
            int got = 0;
            while (ok && got < want && now_ms() < t_end) {
                bool any = false;
                for (auto& kv : listeners) {
                    Receipt r;
                    while (kv.second->try_next_receipt(&r, 0)) {
                        const std::string name = out + "/r" + std::to_string(round) + "_reply_mp" +
                                                 std::to_string(r.model_part) + "_port" + std::to_string(kv.first) + "_" +
                                                 std::to_string(seen[{r.model_part, kv.first}]++) + ".pt";
                        std::ofstream f(name, std::ios::binary);
                        f.write((const char*)r.blob(), (std::streamsize)r.blob_len);
                        ++got;
                        any = true;
                    }
                }
                if (!any) std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
            replies += got;
            if (got < want) {
                std::cerr << "round " << round << " phase " << phase << ": " << got << " of " << want << " replies\n";
                ok = false;
            }
        }
    }
    printf("{\"replies\": %d}\n", replies);
    for (auto& kv : listeners) kv.second->stop();
    return ok ? 0 : 1;
}
