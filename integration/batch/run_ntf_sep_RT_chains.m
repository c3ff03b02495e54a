function B_last = run_ntf_sep_RT_chains(chains, B_DFT_x, B_DFT_d, p, S, chunk_hops)
% run_ntf_sep_RT_chains  The per-target loop of Do_MultiBatch_IS16_20160324.m:183-205 as ONE batched run on the GPU
% (p.NMF_algorithm = 'SNMF', p.B_sep_mode = 'DFT', one channel) through snmf_online_batch_mex
% (integration/snmf_online_batch_mex.cpp, C ABI include/snmf.h: snmf_online_batch_run_chains_*).
%
%   chains      cell array of chains.  A chain is a cell array of {DB_input, DB_output} directory pairs in the order
%               Do_MultiBatch_IS16_20160324.m:186-213 visits them: one noise type, its SNR directories in turn.  The
%               files of a chain are enhanced one after the other; the first starts from B_DFT_d (the
%               delete('B_D_u.mat') of :187), every later one from the dictionary its predecessor adapted.
%   B_DFT_x, B_DFT_d   the event and noise dictionaries every chain starts from
%   p           the settings struct (p.ch = 1); p.precision = 'fp64' selects the fp64 mode
%   S           streams of the batch (chains enhanced at the same time), default min(numel(chains), 256)
%   chunk_hops  hops fed per internal step, default 0 (one device chunk); it changes no bit of the result
%   B_last      F x R_d x numel(chains): every chain's last dictionary, what B_D_u.mat held when the chain ended
% Every chain's last dictionary is also saved as B_D_u_<c>.mat in the directory its last file was written to.
%
% Stated difference from the reference: a chain draws Ad_blk0 (and H0) ONCE and uses them for all its files;
% src/NTF_sep_event_RT.m draws Ad_blk0 again for every file, from the global stream as the previous file left it.
% The first file of a run therefore has the reference's draws; later files of a chain do not.
% This file cannot be executed where the project is built: it is unverified beyond the arity of its MEX calls.

if nargin < 5 || isempty(S), S = min(numel(chains), 256); end
if nargin < 6 || isempty(chunk_hops), chunk_hops = 0; end
if p.ch ~= 1, error('run_ntf_sep_RT_chains:ch', 'one channel only (p.ch = 1)'); end

nc = numel(chains);
R_d = size(B_DFT_d, 2);
r = size(B_DFT_x, 2) + R_d;
pcm = cell(0, 1); n_samples = zeros(0, 1); n_files = zeros(nc, 1); path_out = cell(0, 1); last_dir = cell(nc, 1);
for c = 1:nc
    for d = 1:numel(chains{c})
        DB_input = chains{c}{d}{1}; DB_output = chains{c}{d}{2};
        if ~exist(DB_output, 'dir'), mkdir(DB_output); end
        InFileList = dir(DB_input);                        % run_ntf_sep_RT.m:9-41
        for j = 3:p.filegap:length(InFileList)
            file_name = InFileList(j).name;
            path_denoise = [DB_output, '/', file_name];
            f_tmp = fopen(path_denoise);
            if f_tmp ~= -1
                fclose(f_tmp);
                if ~p.ForceRewrite, continue; end          % :35-40
            end
            fin = fopen([DB_input, '/', file_name], 'rb');
            fread(fin, 22, 'int16');                       % skip the wav header (src/NTF_sep_event_RT.m:56-59)
            pcm{end+1, 1} = fread(fin, inf, 'int16');      %#ok<AGROW>  doubles
            fclose(fin);
            n_samples(end+1, 1) = numel(pcm{end});         %#ok<AGROW>
            path_out{end+1, 1} = path_denoise;             %#ok<AGROW>
            n_files(c) = n_files(c) + 1;
            last_dir{c} = DB_output;
        end
    end
end

% Every chain's draws, made with MATLAB's own generator in the order integration/NTF_sep_event_RT.m:21-34 documents:
% g.A_d (never read), then Ad_blk0, from the global stream as it stands; then the legacy seed and H0.
Ad_blk0 = zeros(p.R_a, p.m_a * nc);
H0 = zeros(r, nc);
for c = 1:nc
    A_d0 = rand(R_d, p.blk_len_sep);                       %#ok<NASGU>  src/init_buff.m:38
    Ad_blk0(:, (c-1)*p.m_a + (1:p.m_a)) = rand(p.R_a, p.m_a);   % src/init_buff.m:39
end
for c = 1:nc
    if p.random_seed > 0
        rand('seed', p.random_seed);                       %#ok<RAND>  src/sparse_nmf.m:112-114: every call re-seeds
    end
    H0(:, c) = rand(r, 1);                                 % src/sparse_nmf.m:133-134
end
if ~p.adapt_train_N, Ad_arg = []; else, Ad_arg = Ad_blk0; end

h = snmf_online_batch_mex('create', B_DFT_x, B_DFT_d, H0(:, 1), Ad_arg(:, 1:min(end, p.m_a)), p, S);
[x, n_out, B_out] = snmf_online_batch_mex('chains', h, vertcat(pcm{:}), n_samples, n_files, repmat(B_DFT_d, 1, nc), H0, Ad_arg, chunk_hops);
snmf_online_batch_mex('destroy', h);

at = 0; f = 0;
B_last = repmat(B_DFT_d, [1, 1, nc]);
for c = 1:nc
    for i = 1:n_files(c)
        f = f + 1;
        fout = fopen(path_out{f}, 'wb');
        fwrite(fout, x(at + (1:n_out(f))), 'int16');       % src/NTF_sep_event_RT.m:124
        fclose(fout);
        pcm2wav(path_out{f}, p);                           % :159
        at = at + n_out(f);
    end
    if n_files(c) > 0
        B_DFT_d_c = B_out(:, (f-1)*R_d + (1:R_d));
        B_last(:, :, c) = B_DFT_d_c;
        S_out = struct('B_DFT_d', B_DFT_d_c, 'B_Mel_d', B_DFT_d_c);   % DFT mode: the Mel slots hold the DFT bases (:138-140)
        save([last_dir{c}, '/B_D_u_', num2str(c), '.mat'], '-struct', 'S_out');
    end
end
end
