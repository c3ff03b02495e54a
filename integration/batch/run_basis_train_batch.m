function [B_DFT, B_Mel, A_DFT, A_Mel] = run_basis_train_batch(DB_path, dir_Basis_full, DC_freq_set, VAD_set, event_num, B_name, R, p)
% run_basis_train_batch  run_basis_train.m of lordet01/SE_SNMF_NAT with the classes trained TOGETHER on the GPU: same signature,
% same files written (the class's wav, R_<R>.mat) and same outputs, but the assembly of the training signals (:16-57), the
% features, the exemplar columns and both sparse_nmf solves (:58-95) of ALL classes that need training are one 'assemble' and
% one 'train_signals' call of integration/snmf_batch_mex.cpp (C ABI include/snmf.h: snmf_train_signals_assemble_f64,
% snmf_run_basis_train_signals_batch_*).  The training signals stay in HBM between the two.
%
% What the loop over the classes keeps is what needs MATLAB: the test for an existing R_<R>.mat / p.ForceRetrain, dir, randperm
% and p.clip_subsample, wavread, load_anot; then the draws in the reference's order, per class: rng('default'); rng(1);
% randsample(T_k, p.cluster_buff * R) (:80-81) and, unless p.snmf_device_rng is set, the rand(n_atoms, T_k) both sparse_nmf
% calls draw after their re-seed (the same matrix for both).  After the call: the renormalisation (:113-116), MATLAB's own
% kmeans (:118-134), the wav (:96) and the save (:136).
% DC_bin is shared by a call, so classes whose DC_freq_set entries give different DC bins go in one call pair per distinct bin.
% A class that needs no cut by VAD stops READING clips once the kept samples exceed p.train_seq_len_max (the library would not
% use the later ones); a VAD class reads all its clips, since what the VAD keeps is decided on the device.
% Stated differences from the reference, both the library's (include/snmf.h): a clip with no kept sample adds nothing, and a
% clip without a variance makes the call fail instead of training NaN dictionaries.
% This file cannot be executed where the project is built: it is unverified beyond the arity of its MEX calls.
addpath('src');
if ~isfield(p, 'random_seed'), p.random_seed = 1; end
if isfield(p, 'snmf_precision') && ~isempty(p.snmf_precision), p.snmf_precision = char(p.snmf_precision); end
DC_bin_set = floor(DC_freq_set ./ (p.fs / p.fftlength) + 0.5);
mat_of = @(l) [dir_Basis_full{l}, '/', 'R_', num2str(R), '.mat'];
n_atoms = p.cluster_buff * R;
device_rng = isfield(p, 'snmf_device_rng') && p.snmf_device_rng;

% ---- which classes to train, and their clips ------------------------------------------------------------------------------
todo = zeros(1, 0);
for l = 1:event_num
    fid = fopen(mat_of(l));
    if fid ~= -1, fclose(fid); end
    if fid == -1 || p.ForceRetrain, todo(end+1) = l; end %#ok<AGROW>
end
clips = cell(1, event_num); ranges = cell(1, event_num); modes = zeros(1, event_num);
for l = todo
    disp(['------', num2str(l), '-th event train------']);
    if VAD_set(l), modes(l) = 1; elseif p.train_ANOT, modes(l) = 2; end
    listing = dir(DB_path{l});
    order = randperm(length(listing) - 2);              % :17 (the two leading entries are . and ..)
    listing = listing(order + 2);
    kept = 0;
    clips{l} = cell(0, 1); ranges{l} = zeros(2, 0);
    for i = 1:p.clip_subsample:length(listing)
        [filename, ext] = strtok(listing(i).name, '.');
        disp(['Training:', filename]);
        s = wavread([DB_path{l}, '/', filename, ext]) .* 32767;
        s = s(:, 1);
        a = 1; b = length(s);
        if modes(l) == 2
            [a, b] = load_anot(filename, length(s), p);
            a = max(a, 1); b = min(b, length(s));
        elseif modes(l) == 0 && p.train_file_len_max > 0
            b = min(b, p.train_file_len_max);
        end
        clips{l}{end+1, 1} = s;
        ranges{l}(:, end+1) = [a; b];
        kept = kept + (b - a + 1);
        if modes(l) ~= 1 && kept > p.train_seq_len_max, break; end
    end
end

% ---- one call pair per distinct DC bin ---------------------------------------------------------------------------------------
melmat = mel_matrix(p.fs, p.F_order, p.fftlength, 1, p.fs/2)';
col = @(c) cell2mat(cellfun(@(a) double(a(:)), c(:), 'UniformOutput', false));
for bin = unique(DC_bin_set(todo))
    group = todo(DC_bin_set(todo) == bin);
    n = numel(group);
    all_clips = vertcat(clips{group});
    clip_len = cellfun(@numel, all_clips);
    n_clips = cellfun(@numel, clips(group))';
    if any(modes(group) == 2), range = [ranges{group}]; else, range = []; end
    h = snmf_batch_mex('assemble', col(all_clips), clip_len(:), n_clips(:), modes(group)', range, p);
    release = onCleanup(@() snmf_batch_mex('signals_destroy', h));
    n_samples = snmf_batch_mex('signals_info', h);

    pp = p; pp.DCbin = bin;
    T = zeros(n, 1); idx = cell(n, 1); H0 = cell(n, 1);
    for k = 1:n
        T(k) = snmf_dnmf_mex('nframes', n_samples(k), pp);
        rng('default'); rng(1);
        idx{k} = randsample(T(k), n_atoms);                 % :80-81
        if p.train_Exemplar == 0 && ~device_rng
            if p.random_seed > 0, rand('seed', p.random_seed); end %#ok<RAND>
            H0{k} = rand(n_atoms, T(k));
        end
    end
    if p.train_Exemplar == 0 && ~device_rng, H0p = col(H0); else, H0p = []; end
    [BD, BM, AD, AM] = snmf_batch_mex('train_signals', h, col(idx), n_atoms, H0p, p, melmat, bin, []);

    at = 0;
    for k = 1:n
        l = group(k);
        cols = (k - 1) * n_atoms + (1:n_atoms);
        B_DFT_init = BD(:, cols); B_Mel_init = BM(:, cols);
        if p.train_Exemplar == 0
            A_DFT_init = reshape(AD(at + (1:n_atoms * T(k))), n_atoms, T(k));
            A_Mel_init = reshape(AM(at + (1:n_atoms * T(k))), n_atoms, T(k));
            at = at + n_atoms * T(k);
        else
            A_DFT_init = 0; A_Mel_init = 0;
        end
        s_full = snmf_batch_mex('signals_get', h, k);
        wavwrite(s_full ./ 32767, 16000, ['basis/', B_name, '/', num2str(l), '.wav']);   % :96
        % unit columns plus the floor (:113-116)
        B_DFT_init = bsxfun(@rdivide, B_DFT_init, sqrt(sum(B_DFT_init .^ 2))) + 1e-9;
        B_Mel_init = bsxfun(@rdivide, B_Mel_init, sqrt(sum(B_Mel_init .^ 2))) + 1e-9;
        if p.cluster_buff > 1
            % one atom per cluster of the Mel dictionary, the one nearest its centre (:118-128), with MATLAB's own kmeans
            [~, ~, ~, D] = kmeans(B_Mel_init', R, 'distance', 'cityblock', 'emptyaction', 'singleto', 'onlinephase', 'off', 'start', 'cluster');
            [~, nearest] = min(D);
            B_Mel_sub = B_Mel_init(:, nearest); B_DFT_sub = B_DFT_init(:, nearest);
            A_DFT_sub = A_DFT_init(nearest, :); A_Mel_sub = A_Mel_init(nearest, :);
        else
            B_Mel_sub = B_Mel_init; B_DFT_sub = B_DFT_init; A_DFT_sub = A_DFT_init; A_Mel_sub = A_Mel_init;
        end
        save(mat_of(l), 'B_DFT_sub', 'B_Mel_sub', 'A_DFT_sub', 'A_Mel_sub', '-v7.3');   % :136
    end
    clear release                                        % 'signals_destroy'
end

% ---- the outputs, from the files as the reference reads them back (:138-149) --------------------------------------------------
B_DFT = zeros(p.F_DFT_order * (2*p.Splice+1), R * event_num);
B_Mel = zeros(p.F_order * (2*p.Splice+1), R * event_num);
A_DFT_all = cell(1, event_num); A_Mel_all = cell(1, event_num);
for l = 1:event_num
    S = load(mat_of(l));
    B_DFT(:, (l-1)*R + (1:R)) = S.B_DFT_sub;
    B_Mel(:, (l-1)*R + (1:R)) = S.B_Mel_sub;
    A_DFT_all{l} = S.A_DFT_sub; A_Mel_all{l} = S.A_Mel_sub;
end
A_DFT = [A_DFT_all{:}]; A_Mel = [A_Mel_all{:}];
if ~any(A_DFT(:)) && numel(A_DFT) == event_num, A_DFT = 0; A_Mel = 0; end   % train_Exemplar: the reference keeps the scalar 0
fclose('all');
end
