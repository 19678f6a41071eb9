// carmel_ranks.cpp — --gpus=N: N processes, one per GPU, forked before anything touches a GPU.  Every rank reads the same files and
// composes the same cascade; rank r keeps the r-th contiguous block of the training pairs, builds its lattices, and the
// expected counts are summed across ranks once per iteration (carmel_hip_allreduce_counts: RCCL over xGMI, on the
// trainer's stream between the count pass and the M-step).  The M-step is replicated, so every rank holds the same
// weights and takes the same decisions; rank 0 alone logs and writes the results.
// (--crp: the runs of --crp-restarts are independent chains; with --gpus=N rank r takes the runs r, r + N, ... on the whole
// corpus and the ranks agree on the run to keep -- gibbs_base::run_starts with its runs side by side)
#include <dlfcn.h>
#include <signal.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>
#include "carmel_cli.hpp"
using namespace carmel_host;

static std::vector<pid_t> g_kids;  // --gpus: the other ranks (rank 0 only)
static int g_rank = 0;
static int g_err_fd = -1;  // ranks > 0: the job's stderr, for the one message that says why the rank failed
static std::string g_session;  // --comm-plugin: the name the ranks' transports meet under
static std::vector<int> g_id_pipes;  // rank 0: write ends towards the other ranks (the communicator id)
static int g_id_read = -1;           // ranks > 0: the read end
static volatile sig_atomic_t g_waiting = 0;  // rank 0 is in its final waitpid loop (children may exit normally)
// A rank that dies leaves the others waiting in a collective for ever (RCCL blocks; round-2 advisor finding): rank 0
// watches its children and ends the whole job the moment one of them exits abnormally.
static void on_sigchld(int) {
  if (g_waiting) return;
  int st = 0;
  for (pid_t p : g_kids) {
    const pid_t r = waitpid(p, &st, WNOHANG);
    if (r == p && (!WIFEXITED(st) || WEXITSTATUS(st) != 0)) {
      static const char msg[] = "ERROR: a rank of --gpus ended abnormally; ending the job\n";
      if (write(2, msg, sizeof msg - 1) < 0) {}
      for (pid_t q : g_kids)
        if (q != p) kill(q, SIGTERM);
      _exit(245);  // -11
    }
  }
}

// forks ranks 1 .. world-1 (j.rank says which one returns); false: a rank could not drop its streams
bool fork_ranks(Job& j) {
  const Options& o = j.o;
  const int world = j.world;
  int& rank = j.rank;
  if (world > 1 && (!o.fem_forest.empty() || !o.fem_norm.empty() || !o.fem_param.empty() || !o.fem_alpha.empty()))
    throw UsageError("--gpus with the --fem-* exports is not supported (the export walks the whole corpus)");
  if (world > 1) {
    {
      char buf[96];
      std::snprintf(buf, sizeof buf, "carmel_%d_%ld", (int)getpid(), (long)time(nullptr));
      g_session = buf;
    }
    for (int r = 1; r < world; ++r) {
      int fd[2];
      if (pipe(fd) != 0) throw std::runtime_error("pipe() failed");
      pid_t pid = fork();
      if (pid < 0) throw std::runtime_error("fork() failed");
      if (pid == 0) {
        rank = r;
        close(fd[1]);
        g_id_read = fd[0];
        for (int w : g_id_pipes) close(w);
        g_id_pipes.clear();
        g_kids.clear();
        // a rank other than 0 says nothing unless something goes wrong (its log lines are rank 0's): its streams are dropped, but
        // a copy of stderr is kept for the reason it died, should it die; and no rank outlives rank 0
        g_err_fd = dup(2);
        if (!std::freopen("/dev/null", "w", stdout) || !std::freopen("/dev/null", "w", stderr)) return false;
        prctl(PR_SET_PDEATHSIG, SIGTERM);
        g_rank = r;
        break;
      }
      close(fd[0]);
      g_id_pipes.push_back(fd[1]);
      g_kids.push_back(pid);
    }
    if (rank == 0) {
      struct sigaction sa;
      std::memset(&sa, 0, sizeof sa);
      sa.sa_handler = on_sigchld;
      sa.sa_flags = SA_RESTART | SA_NOCLDSTOP;
      sigaction(SIGCHLD, &sa, nullptr);
    }
  } else if (o.gpus > 1)
    std::cerr << "--gpus=" << o.gpus << " applies to EM training (-t / --train-cascade) and to the runs of --crp --crp-restarts=R; running on one GPU\n";
  return true;
}

// --comm-plugin: the plugin exports  int carmel_hip_transport_open(const char* session, int rank, int world, int device,
// carmel_hip_transport* out);  the session name is the same on every rank (made before the ranks were forked)
static void create_plugin_communicator(Job& j, int my_device) {
  const Options& o = j.o;
  void* h = dlopen(o.comm_plugin.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!h) throw std::runtime_error(std::string("--comm-plugin: ") + dlerror());
  typedef int (*open_fn)(const char*, int, int, int, carmel_hip_transport*);
  open_fn op = (open_fn)dlsym(h, "carmel_hip_transport_open");
  if (!op) throw std::runtime_error("--comm-plugin: the library does not export carmel_hip_transport_open");
  carmel_hip_transport tr;
  std::memset(&tr, 0, sizeof tr);
  if (op(g_session.c_str(), j.rank, j.world, my_device, &tr) != 0) throw std::runtime_error("--comm-plugin: carmel_hip_transport_open failed");
  hip_check(carmel_hip_comm_create_custom(&j.comm, my_device, j.rank, j.world, &tr), "carmel_hip_comm_create_custom");
  if (carmel_hip_sendrecv_fn sr = (carmel_hip_sendrecv_fn)dlsym(h, "carmel_hip_transport_sendrecv"))  // optional: point-to-point groups
    hip_check(carmel_hip_comm_set_sendrecv(j.comm, sr), "carmel_hip_comm_set_sendrecv");
  for (int w : g_id_pipes) close(w);
  if (g_id_read >= 0) close(g_id_read);
}

void create_communicator(Job& j, int my_device) {
  if (j.world > 1 && !j.o.comm_plugin.empty()) {
    create_plugin_communicator(j, my_device);
  } else if (j.world > 1) {  // rank 0 makes the communicator's id and hands it to the others through their pipes
    unsigned char id[128];
    if (j.rank == 0) {
      hip_check(carmel_hip_comm_unique_id(id), "carmel_hip_comm_unique_id");
      for (int w : g_id_pipes) {
        if (write(w, id, sizeof id) != (ssize_t)sizeof id) throw std::runtime_error("could not hand the communicator id to a rank");
        close(w);
      }
    } else {
      size_t got = 0;
      while (got < sizeof id) {
        ssize_t n = read(g_id_read, id + got, sizeof id - got);
        if (n <= 0) throw std::runtime_error("rank 0 went away before the communicator id arrived");
        got += (size_t)n;
      }
      close(g_id_read);
    }
    hip_check(carmel_hip_comm_create(&j.comm, my_device, j.rank, j.world, id), "carmel_hip_comm_create");
  }
}

void shard_pairs(Job& j) {  // this rank's block of the training pairs
  HostPairs& pairs = j.pairs;
  const int rank = j.rank, world = j.world;
  const size_t n = pairs.size(), lo = n * (size_t)rank / (size_t)world, hi = n * (size_t)(rank + 1) / (size_t)world;
  HostPairs mine;
  mine.in_off.assign(1, 0);
  mine.out_off.assign(1, 0);
  for (size_t p = lo; p < hi; ++p) {
    mine.in_sym.insert(mine.in_sym.end(), pairs.in_sym.begin() + pairs.in_off[p], pairs.in_sym.begin() + pairs.in_off[p + 1]);
    mine.out_sym.insert(mine.out_sym.end(), pairs.out_sym.begin() + pairs.out_off[p], pairs.out_sym.begin() + pairs.out_off[p + 1]);
    mine.in_off.push_back(mine.in_sym.size());
    mine.out_off.push_back(mine.out_sym.size());
    mine.weight.push_back(pairs.weight[p]);
  }
  pairs = mine;
  if (!j.quiet) std::cerr << "Corpus sharded over " << world << " GPUs: rank 0 keeps " << pairs.size() << " of " << n << " pairs\n";
}

void report_error(const char* what) {
  if (g_rank && g_err_fd >= 0)
    dprintf(g_err_fd, "[rank %d] ERROR: %s\n", g_rank, what);
  else
    std::cerr << "ERROR: " << what << "\n";  // carmel.cc:1558-1561
}

// --gpus: rank 0 waits for the other ranks; if it failed itself they may be waiting in a collective -- end them
int wait_for_ranks(int rc) {
  g_waiting = 1;
  for (pid_t p : g_kids) {
    if (rc != 0) kill(p, SIGTERM);
    int st = 0;
    if (waitpid(p, &st, 0) > 0 && (!WIFEXITED(st) || WEXITSTATUS(st) != 0) && rc == 0) rc = -11;
  }
  return rc;
}
